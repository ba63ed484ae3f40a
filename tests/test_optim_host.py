"""CPU: the host side of the native training loop -- schedules against torch.optim.lr_scheduler,
the train / validation split against scikit-learn, create_optimizer's argument checks, the
checkpoint layout, flat parameters as a pure re-pointing, and the new symbol in the ABI."""
import re

import pytest
import torch

from tests.conftest import ROOT

LR = 1e-3
SCHEDULES = {
    "exp": ("exp", dict(gamma=0.99), torch.optim.lr_scheduler.ExponentialLR),
    "cosine": ("cosine", dict(T_max=25, eta_min=1e-5), torch.optim.lr_scheduler.CosineAnnealingLR),
    "cosine_to_zero": ("cosine", dict(T_max=25), torch.optim.lr_scheduler.CosineAnnealingLR),
    "cosine_warmup": ("cosine_warmup", dict(T_0=9), torch.optim.lr_scheduler.CosineAnnealingWarmRestarts),
    "cosine_warmup_mult": ("cosine_warmup", dict(T_0=7, T_mult=2, eta_min=1e-6),
                           torch.optim.lr_scheduler.CosineAnnealingWarmRestarts),
    "onecycle": ("onecycle", dict(max_lr=1e-2, total_steps=61), torch.optim.lr_scheduler.OneCycleLR),
    "onecycle_three_linear": ("onecycle", dict(max_lr=1e-2, total_steps=61, three_phase=True, anneal_strategy="linear",
                                               pct_start=0.25), torch.optim.lr_scheduler.OneCycleLR),
    "onecycle_epochs": ("onecycle", dict(max_lr=3e-3, epochs=61, steps_per_epoch=1, cycle_momentum=False),
                        torch.optim.lr_scheduler.OneCycleLR),
}


@pytest.mark.parametrize("case", sorted(SCHEDULES))
def test_schedule_matches_torch(case):
    """60 scheduler steps, one per epoch as Lightning takes them, to 1e-12 relative."""
    from learningsparsepreconditioner4gpu_amd.optim import create_scheduler

    name, kw, cls = SCHEDULES[case]
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=LR)
    ref = cls(opt, **kw)
    mine = create_scheduler(name, kw, base_lr=LR)
    for t in range(61):
        want = opt.param_groups[0]["lr"]
        got = mine.lr(t)
        assert abs(got - want) <= 1e-12 * abs(want), (case, t, got, want)
        mom = mine.momentum(t)
        if name == "onecycle" and kw.get("cycle_momentum", True):
            assert abs(mom - opt.param_groups[0]["betas"][0]) <= 1e-12, (case, t)
        else:
            assert mom is None
        if t < 60:
            opt.step()
            ref.step()


def test_scheduler_names():
    from learningsparsepreconditioner4gpu_amd.optim import create_scheduler

    assert create_scheduler("none", {}) is None
    with pytest.raises(ValueError, match="Unknown scheduler"):
        create_scheduler("plateau", {})
    with pytest.raises(TypeError):
        create_scheduler("exp", dict(gamma=0.9, verbose=True))
    with pytest.raises(ValueError):
        create_scheduler("onecycle", dict(max_lr=1e-2))  # neither total_steps nor epochs x steps_per_epoch


def test_split_matches_sklearn():
    from learningsparsepreconditioner4gpu_amd.optim import _split_restated, train_val_split

    # RandomState(42).permutation(10) = [8 1 5 0 7 2 9 4 3 6]
    assert _split_restated(10, 0.8) == ([5, 0, 7, 2, 9, 4, 3, 6], [8, 1])
    assert train_val_split(10, 0.8)[1] == [8, 1]
    try:
        from sklearn.model_selection import train_test_split
    except ImportError:
        train_test_split = None
    for n in (2, 5, 10, 37):
        for r in (0.8, 0.5):
            tr, va = _split_restated(n, r)
            assert sorted(tr + va) == list(range(n)) and len(tr) == int(r * n)
            assert train_val_split(n, r) == (tr, va)
            if train_test_split is not None:
                want = train_test_split(range(n), train_size=r, random_state=42, shuffle=True)
                assert (tr, va) == (list(want[0]), list(want[1])), (n, r)
    with pytest.raises(ValueError):
        _split_restated(1, 0.8)


def test_create_optimizer_arguments():
    from learningsparsepreconditioner4gpu_amd.optim import create_optimizer

    o = create_optimizer("adamw", {"lr": 2e-3, "weight_decay": 3e-3}, clip_norm=10, accumulate=4)
    assert (o.name, o.lr, o.weight_decay, o.betas, o.eps) == ("adamw", 2e-3, 3e-3, (0.9, 0.999), 1e-8)
    assert o.clip_norm == 10.0 and o.grad_scale == 0.25 and o.uses_m and o.uses_v
    assert create_optimizer("adamw").weight_decay == 1e-2 and create_optimizer("adam").weight_decay == 0.0  # torch's
    s = create_optimizer("sgd", {"lr": 0.1})
    assert not s.uses_m and not s.uses_v and s.clip_norm == 0.0
    assert create_optimizer("sgd", {"lr": 0.1, "momentum": 0.9, "nesterov": False, "dampening": 0}).uses_m
    with pytest.raises(ValueError, match="Unknown optimizer"):
        create_optimizer("rmsprop", {})
    for name, bad in (("adam", {"amsgrad": True}), ("adamw", {"maximize": True}),
                      ("sgd", {"momentum": 0.9, "nesterov": True}), ("sgd", {"momentum": 0.9, "dampening": 0.1})):
        with pytest.raises(NotImplementedError):
            create_optimizer(name, bad)
    with pytest.raises(TypeError):
        create_optimizer("sgd", {"betas": (0.9, 0.99)})
    with pytest.raises(ValueError):
        create_optimizer("adam", {"lr": -1.0})


def test_optimizer_state_round_trip():
    from learningsparsepreconditioner4gpu_amd.optim import create_optimizer

    a = create_optimizer("adamw", {"lr": 1e-3})
    a.load_state_dict({"kind": "adamw", "step": 7, "m": torch.arange(5.0), "v": torch.ones(5), "betas": [0.85, 0.999],
                       "momentum": 0.0})
    sd = a.state_dict()
    assert sd["step"] == 7 and sd["betas"] == [0.85, 0.999]
    assert torch.equal(sd["m"], torch.arange(5.0)) and torch.equal(sd["v"], torch.ones(5))
    with pytest.raises(ValueError):
        create_optimizer("sgd", {"lr": 1e-3}).load_state_dict(sd)


def test_checkpoint_round_trip(tmp_path):
    from learningsparsepreconditioner4gpu_amd.optim import create_optimizer
    from learningsparsepreconditioner4gpu_amd.workspace import (ScaledInferenceWorkspace, SimpleInferenceWorkspace,
                                                                load_checkpoint_weights_only)

    ws = ScaledInferenceWorkspace(node_features=3, edge_features=2, block_size=1, epsilon=2e-3, seed=5, device="cpu",
                                  loss_name="L2Loss_ANorm")
    opt = create_optimizer("adamw", {"lr": 1e-3})
    opt.load_state_dict({"kind": "adamw", "step": 3, "m": torch.full((4,), 0.5), "v": torch.full((4,), 0.25)})
    hp = {"optimizer": {"name": "adamw", "params": {"lr": 1e-3}}, "scheduler": {"name": "exp", "params": {"gamma": 0.99}},
          "batch_size": 4}
    path = ws.save_checkpoint(tmp_path / "sub" / "a.ckpt", epoch=4, global_step=11, optimizer=opt, hparams=hp)
    assert ws.last_checkpoint == path
    ck = load_checkpoint_weights_only(path)
    assert set(ck) == {"state_dict", "hyper_parameters", "epoch", "global_step", "native_optimizer", "workspace"}
    assert set(ck["hyper_parameters"]) == {"node_features", "edge_features", "block_size", "epsilon", "gnn", "loss",
                                           "optimizer", "scheduler", "batch_size"}
    assert (ck["epoch"], ck["global_step"], ck["workspace"]) == (4, 11, "scaled")
    assert ck["hyper_parameters"]["loss"] == {"name": "L2Loss_ANorm", "params": {}}
    assert ck["native_optimizer"]["kind"] == "adamw" and ck["native_optimizer"]["step"] == 3
    assert torch.equal(ck["native_optimizer"]["v"], torch.full((4,), 0.25))
    assert all(k.startswith("gnn.") for k in ck["state_dict"])
    back = ScaledInferenceWorkspace.load_from_checkpoint(path, device="cpu")
    assert back.epsilon == 2e-3 and back.loss_name == "L2Loss_ANorm" and back.gnn_config == ws.gnn_config
    want = ws.gnn.state_dict()
    got = back.gnn.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    # the base class reads it too (infer picks the class from its own flag)
    SimpleInferenceWorkspace.load_from_checkpoint(path, device="cpu")


def test_flatten_parameters_is_a_repointing():
    from learningsparsepreconditioner4gpu_amd.nn import build_gnn

    plain = build_gnn(3, 2, 1, seed=4)
    flat = build_gnn(3, 2, 1, seed=4)
    assert not flat.is_flat()
    host = plain.pack_weights()
    blob = flat.flatten_parameters("cpu")
    assert flat.is_flat() and flat.pack_weights() is blob and torch.equal(blob, host)
    want, got = plain.state_dict(), flat.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    # an in-place write to the blob is the parameters' new value, and load_state_dict writes through
    blob.mul_(2.0)
    assert all(torch.equal(flat.state_dict()[k], 2 * want[k]) for k, _ in flat._packed_params())
    flat.load_state_dict(want)
    assert flat.is_flat() and torch.equal(blob, host)
    # re-allocating the parameters ends the flat state; packing works as before
    flat.double()
    assert not flat.is_flat() and torch.equal(flat.pack_weights(), host)


def test_symbol_declared_and_bound():
    from learningsparsepreconditioner4gpu_amd import _build, _lib

    header = (ROOT / "include" / "lspcg.h").read_text()
    assert re.search(r"\bint lspcg_optim_step\(lspcg_ctx\* ctx, const lspcg_optim_desc\* desc,", header)
    for kind, code in _lib.OPT_KIND.items():
        assert re.search(rf"#define LSPCG_OPT_{kind.upper()} {code}\b", header)
    assert "lspcg_optim_step" in _lib.SIGNATURES and len(_lib.SIGNATURES["lspcg_optim_step"][1]) == 10
    assert [n for n, _ in _lib.lspcg_optim_desc._fields_] == ["kind", "beta1", "beta2", "eps", "weight_decay",
                                                             "momentum", "clip_norm", "grad_scale"]
    assert "lspcg_optim.hip" in _build.SOURCES
    # the workgroup size the GPU tests place their sizes around
    assert "kOptThreads = 1024" in (_build.CSRC / "lspcg_optim.hip").read_text()
