"""Training driver: the reference's ``train.py`` + Lightning ``Trainer.fit`` on the HIP kernels.

``fit(ws, dataset, ...)`` (also ``ws.fit``) is the epoch loop: the reference's train / validation
split (``neural_cg/utils/datamodule.py:26``), shuffled batches of ``batch_size`` graphs collated
into one disjoint union, per batch ``ws.fit_step`` -- ``lspcg_gnn_forward``, the fused loss and its
gradient, ``lspcg_gnn_backward``, ``lspcg_optim_step``, ``lspcg_gnn_set_weights``; no autograd
graph, no per-parameter tensors -- a learning-rate schedule stepped once per epoch as Lightning
does, validation every ``check_val_every_n_epoch`` epochs and a checkpoint every
``checkpoint_every_n_epochs``.  Losses stay on the device and are read once per epoch.

    python -m learningsparsepreconditioner4gpu_amd.train --synthetic heat_batch8 --epochs 20 --out runs/heat
    python -m learningsparsepreconditioner4gpu_amd.train --dataset generated/heat --config my.yaml --out runs/heat
    python -m learningsparsepreconditioner4gpu_amd.infer --dataset heat_batch8 --checkpoint runs/heat/checkpoints/epoch=19.ckpt

Not here (the reference has them): MLflow logging, Hydra composition (``--config`` reads ONE user
yaml in the reference's key layout), the multi-folder datamodule, data-parallel training.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Optional, Sequence

import torch

from .data import GraphSample, collate
from .optim import NativeOptimizer, create_optimizer, create_scheduler, train_val_split

# The reference's defaults, as constants (no yaml is shipped):
BATCH_SIZE = 4                      # config/basic.yaml:9
SEED = 42                           # config/basic.yaml:15
SPLIT_TRAIN = 0.8                   # config/trainer.yaml:2
OPTIMIZER = {"name": "adamw", "params": {"lr": 1e-3, "weight_decay": 3e-3}}  # config/trainer.yaml:8-12
SCHEDULER = {"name": "exp", "params": {"gamma": 0.99}}                       # config/trainer.yaml:13-16
MAX_EPOCHS = 500                    # config/trainer.yaml:19
CHECK_VAL_EVERY_N_EPOCH = 5         # config/trainer.yaml:20
ACCUMULATE_GRAD_BATCHES = 1         # config/trainer.yaml:21
GRADIENT_CLIP_VAL = 10              # config/trainer.yaml:22
CHECKPOINT_EVERY_N_EPOCHS = 1       # config/trainer.yaml:25-26


def _plain_cfg(o):
    if isinstance(o, dict):
        return {str(k): _plain_cfg(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain_cfg(v) for v in o]
    return o


def workspace_kind(ws) -> str:
    from .workspace import ScaledInferenceWorkspace

    return "scaled" if isinstance(ws, ScaledInferenceWorkspace) else "simple"


def save_checkpoint(ws, path, epoch: int = 0, global_step: int = 0, optimizer: Optional[NativeOptimizer] = None,
                    hparams: Optional[dict] = None) -> str:
    """A checkpoint in the reference's (Lightning's) key layout, holding plain dicts and tensors only,
    so ``load_checkpoint_weights_only`` / ``load_from_checkpoint`` read it without any allowlist:
    ``state_dict`` (``gnn.*``), ``hyper_parameters`` (node_features, edge_features, block_size,
    epsilon, gnn, loss{name, params}, plus ``hparams``: optimizer, scheduler, batch_size), ``epoch``
    (the index of the last finished epoch, Lightning's convention), ``global_step``,
    ``native_optimizer`` (``NativeOptimizer.state_dict()``) and ``workspace`` (simple | scaled).
    Copies the weights and the optimizer state to the host (synchronises)."""
    hp = {"node_features": ws.node_features, "edge_features": ws.edge_features, "block_size": int(ws.block_size),
          "epsilon": float(ws.epsilon), "gnn": _plain_cfg(ws.gnn_config),
          "loss": {"name": ws.loss_name, "params": _plain_cfg(ws.loss_params)}}
    hp.update(_plain_cfg(hparams or {}))
    # parameters of a flattened module are views of one blob: clone, or every entry would carry all of it
    sd = {"gnn." + k: v.detach().cpu().clone() for k, v in ws.gnn.state_dict().items()}
    ck = {"state_dict": sd, "hyper_parameters": hp, "epoch": int(epoch), "global_step": int(global_step),
          "native_optimizer": None if optimizer is None else optimizer.state_dict(), "workspace": workspace_kind(ws)}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(ck, str(path))
    ws.last_checkpoint = str(path)
    return str(path)


def _val_loss(ws, samples: Sequence[GraphSample]) -> torch.Tensor:
    """The mean of ``shared_step``'s loss over ``samples`` at batch size 1 (datamodule.py:57), on the device."""
    return torch.stack([ws.shared_step(s)[1].double() for s in samples]).mean()


def _converge_iters(ws, sample: GraphSample) -> float:
    """``Val/cuda_neural_iter``: PCG iterations with the current L on one sample, rhs = mask
    (workspace.py:136, 162)."""
    from .validate import get_pcg_iter_time, get_pcg_scaled_iter_time

    pcg = get_pcg_scaled_iter_time if workspace_kind(ws) == "scaled" else get_pcg_iter_time
    L, _ = ws.inference_step(sample)
    r = sample.mask.detach().cpu().numpy().reshape(-1).astype("float64")
    return float(pcg(ws.system_matrix(sample), r, L, ws.epsilon, device="cuda")[0])


def _converge_cond(ws, sample: GraphSample) -> float:
    """``Val/cuda_neural_cond``: κ(M⁻¹A) with the current L on the same sample, from a solve of its
    own with a random start (``ws.condition_number``: the mask is no start for a spectrum estimate)."""
    return float(ws.condition_number(sample, "neural").cond)


def fit(ws, dataset: Sequence[GraphSample], batch_size: int = BATCH_SIZE, max_epochs: int = MAX_EPOCHS,
        split_train: float = SPLIT_TRAIN, check_val_every_n_epoch: int = CHECK_VAL_EVERY_N_EPOCH,
        accumulate_grad_batches: int = ACCUMULATE_GRAD_BATCHES, gradient_clip_val: Optional[float] = GRADIENT_CLIP_VAL,
        optimizer: Optional[dict] = None, scheduler: Optional[dict] = None, seed: int = SEED,
        out_dir: Optional[str] = None, checkpoint_every_n_epochs: int = CHECKPOINT_EVERY_N_EPOCHS,
        check_converge: bool = False, resume: Optional[str] = None, verbose: bool = False,
        val_cond: bool = False) -> list:
    """Train ``ws.gnn`` on ``dataset`` (samples built with ``is_inference=False``; anything with
    ``len`` and integer indexing; each sample is moved to the device on first use and kept there).
    Defaults are the reference's (the constants above).

    * split: ``train_test_split(range(n), train_size=split_train, random_state=42, shuffle=True)``;
      the training order of epoch ``e`` is ``torch.randperm`` from a generator seeded ``seed + e``.
    * the schedule is stepped per epoch: epoch ``e`` trains with ``lr(e)``.
    * every ``check_val_every_n_epoch`` epochs ``Val/Loss`` is the mean loss over the validation
      samples at batch size 1; with ``check_converge`` the first one also gives
      ``Val/cuda_neural_iter`` (PCG with the current L, rhs = mask); with ``val_cond`` it also gives
      ``Val/cuda_neural_cond``, the condition number of the preconditioned system estimated from a
      separate solve with a random start (``spectrum.condition_number``, rtol 1e-8).
    * one dict per epoch goes to ``ws.history`` (returned) and, with ``out_dir``, to
      ``out_dir/metrics.jsonl``; checkpoints to ``out_dir/checkpoints/epoch=NN.ckpt`` every
      ``checkpoint_every_n_epochs`` epochs and after the last one (``ws.last_checkpoint``).
    * ``resume``: a checkpoint of this function; weights, optimizer state, epoch and step are
      restored and the run continues with the bits an uninterrupted one would have.
    """
    from .workspace import load_checkpoint_weights_only

    opt_cfg = _plain_cfg(optimizer if optimizer is not None else OPTIMIZER)
    sch_cfg = _plain_cfg(scheduler if scheduler is not None else SCHEDULER)
    n = len(dataset)
    train_idx, val_idx = train_val_split(n, split_train)
    opt = create_optimizer(opt_cfg["name"], opt_cfg.get("params"), clip_norm=gradient_clip_val,
                           accumulate=accumulate_grad_batches)
    sched = create_scheduler(sch_cfg["name"], sch_cfg.get("params"), base_lr=opt.lr)
    start_epoch, global_step = 0, 0
    if resume:
        ck = load_checkpoint_weights_only(str(resume))
        if ck.get("native_optimizer") is None:
            raise ValueError(f"{resume} holds no native_optimizer state to resume from")
        ws.gnn.load_state_dict({k[len("gnn."):]: v for k, v in ck["state_dict"].items() if k.startswith("gnn.")})
        opt.load_state_dict(ck["native_optimizer"])
        start_epoch, global_step = int(ck["epoch"]) + 1, int(ck["global_step"])
    else:
        ws.history = []
    ws.gnn.flatten_parameters(ws.device)
    cache = {}

    def sample(i: int) -> GraphSample:
        if i not in cache:
            cache[i] = dataset[i].to(ws.device)
        return cache[i]

    hparams = {"optimizer": opt_cfg, "scheduler": sch_cfg, "batch_size": int(batch_size)}
    out = None if out_dir is None else Path(out_dir)
    if out is not None:
        out.mkdir(parents=True, exist_ok=True)
    for epoch in range(start_epoch, max_epochs):
        lr = opt.lr if sched is None else sched.lr(epoch)
        mom = None if sched is None else sched.momentum(epoch)
        if mom is not None:
            opt.set_momentum(mom)
        order = torch.randperm(len(train_idx), generator=torch.Generator().manual_seed(seed + epoch)).tolist()
        losses, sizes = [], []
        for k in range(0, len(order), batch_size):
            chunk = [train_idx[j] for j in order[k:k + batch_size]]
            losses.append(ws.fit_step(collate([sample(i) for i in chunk]), opt, lr).double())
            sizes.append(len(chunk))
            global_step += 1
        opt.flush(ws.gnn, lr)
        # the epoch's only host reads: the batch losses (weighted by their graph counts) and the last step's norms
        wts = torch.tensor(sizes, dtype=torch.float64, device=losses[0].device)
        row = {"epoch": epoch, "global_step": global_step, "lr": lr,
               "Train/Loss": float((torch.stack(losses) * wts).sum() / wts.sum())}
        if opt.stats is not None:
            st = opt.stats.tolist()
            row["Train/total_grad_norm"], row["Train/total_param_norm"] = st[0], st[2]
        if check_val_every_n_epoch and (epoch + 1) % check_val_every_n_epoch == 0 and val_idx:
            row["Val/Loss"] = float(_val_loss(ws, [sample(i) for i in val_idx]))
            if check_converge:
                row["Val/cuda_neural_iter"] = _converge_iters(ws, sample(val_idx[0]))
            if val_cond:
                row["Val/cuda_neural_cond"] = _converge_cond(ws, sample(val_idx[0]))
        ws.history.append(row)
        if out is not None:
            with open(out / "metrics.jsonl", "a") as f:
                f.write(json.dumps(row) + "\n")
            if (checkpoint_every_n_epochs and (epoch + 1) % checkpoint_every_n_epochs == 0) or epoch == max_epochs - 1:
                save_checkpoint(ws, out / "checkpoints" / f"epoch={epoch:02d}.ckpt", epoch=epoch,
                                global_step=global_step, optimizer=opt, hparams=hparams)
        if verbose:
            print(" ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    ws.optimizer = opt
    return ws.history


# ---------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------
def _load_config(path: Optional[str]) -> dict:
    if not path:
        return {}
    import yaml

    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: expected a mapping at the top level")
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the SPAI GNN on the GPU (HIP kernels end to end).")
    ap.add_argument("--dataset", default=None, help="prefix of an on-disk dataset (dataset.FolderDataset)")
    ap.add_argument("--synthetic", default=None, help="a stand-in set of infer.synthetic_dataset, e.g. heat_batch8")
    ap.add_argument("--workspace", default=None, choices=["simple", "scaled"])
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--weight-decay", type=float, default=None)
    ap.add_argument("--scheduler", default=None, choices=["exp", "cosine", "cosine_warmup", "onecycle", "none"])
    ap.add_argument("--gamma", type=float, default=None, help="gamma of the exp schedule")
    ap.add_argument("--clip", type=float, default=None, help="gradient_clip_val (0: off)")
    ap.add_argument("--accumulate", type=int, default=None)
    ap.add_argument("--loss", default=None, help="RelativeL2Loss_ANorm | L2Loss_ANorm")
    ap.add_argument("--out", default=None, help="directory for metrics.jsonl and checkpoints/")
    ap.add_argument("--resume", default=None, help="a checkpoint of this program to continue from")
    ap.add_argument("--config", default=None,
                    help="a yaml file in the reference's key layout (batch_size, epsilon, seed, workspace, split.train, "
                         "optimizer, scheduler, trainer.*, checkpoint.every_n_epochs, loss, data); flags override it")
    ap.add_argument("--check-converge", action="store_true")
    ap.add_argument("--val-cond", action="store_true",
                    help="log Val/cuda_neural_cond: the condition number of M^-1 A on the first validation sample")
    args = ap.parse_args(argv)
    cfg = _load_config(args.config)
    pick = lambda flag, *keys, default=None: flag if flag is not None else _dig(cfg, keys, default)

    from .infer import synthetic_dataset
    from .nn import _weight_init
    from .workspace import ScaledInferenceWorkspace, SimpleInferenceWorkspace

    seed = int(_dig(cfg, ("seed",), SEED))
    prefix = pick(args.dataset, "data", "prefix")
    if args.synthetic:
        samples = synthetic_dataset(args.synthetic, is_inference=False)
    elif prefix:
        from .dataset import FolderDataset

        d = dict(is_fixed_topology=False, load_into_memory=False, block_size=1, has_shared_features=False,
                 use_node_features=True, use_matrix_as_edge_feature=True, use_mask_as_node_feature=True,
                 use_node_features_as_edge_feature=False, use_edge_features_as_node_feature="disable",
                 use_random_rhs=True, normalize_matrix="mean")  # config/data.yaml
        d.update({k: v for k, v in (cfg.get("data") or {}).items() if k in d})
        ds = FolderDataset(prefix=prefix, **d)
        torch.manual_seed(seed)
        samples = [ds.get(i, is_inference=False) for i in range(ds.len())]
    else:
        ap.error("one of --dataset PREFIX (or data.prefix in --config) and --synthetic NAME is needed")
    kind = pick(args.workspace, "workspace", default="simple")
    if args.resume and args.workspace is None:
        from .workspace import load_checkpoint_weights_only

        kind = load_checkpoint_weights_only(args.resume).get("workspace", kind)
    cls = ScaledInferenceWorkspace if kind == "scaled" else SimpleInferenceWorkspace
    loss_cfg = cfg.get("loss") or {}
    loss_name = pick(args.loss, "loss", "name", default="RelativeL2Loss_ANorm")
    s0 = samples[0]
    if args.resume:
        ws = cls.load_from_checkpoint(args.resume)
    else:
        ws = cls(node_features=s0.x.shape[1], edge_features=s0.edge_attr.shape[1], block_size=s0.block_size,
                 epsilon=float(_dig(cfg, ("epsilon",), 3e-3)), gnn=cfg.get("gnn"), seed=seed, loss_name=loss_name,
                 loss_params=loss_cfg.get("params") if args.loss is None else None)
        ws.gnn.apply(_weight_init)  # train.py:70 model.apply(weight_init)
    optimizer = _plain_cfg(cfg.get("optimizer") or OPTIMIZER)
    optimizer["params"] = dict(optimizer.get("params") or {})
    if args.lr is not None:
        optimizer["params"]["lr"] = args.lr
    if args.weight_decay is not None:
        optimizer["params"]["weight_decay"] = args.weight_decay
    scheduler = _plain_cfg(cfg.get("scheduler") or SCHEDULER)
    if args.scheduler is not None and args.scheduler != scheduler.get("name"):
        scheduler = {"name": args.scheduler, "params": {}}
    scheduler["params"] = dict(scheduler.get("params") or {})
    if args.gamma is not None:
        scheduler["params"]["gamma"] = args.gamma
    history = fit(ws, samples,
                  batch_size=int(pick(args.batch_size, "batch_size", default=BATCH_SIZE)),
                  max_epochs=int(pick(args.epochs, "trainer", "max_epochs", default=MAX_EPOCHS)),
                  split_train=float(_dig(cfg, ("split", "train"), SPLIT_TRAIN)),
                  check_val_every_n_epoch=int(_dig(cfg, ("trainer", "check_val_every_n_epoch"), CHECK_VAL_EVERY_N_EPOCH)),
                  accumulate_grad_batches=int(pick(args.accumulate, "trainer", "accumulate_grad_batches",
                                                   default=ACCUMULATE_GRAD_BATCHES)),
                  gradient_clip_val=float(pick(args.clip, "trainer", "gradient_clip_val", default=GRADIENT_CLIP_VAL)),
                  optimizer=optimizer, scheduler=scheduler, seed=seed, out_dir=args.out,
                  checkpoint_every_n_epochs=int(_dig(cfg, ("checkpoint", "every_n_epochs"), CHECKPOINT_EVERY_N_EPOCHS)),
                  check_converge=bool(args.check_converge), resume=args.resume, verbose=True,
                  val_cond=bool(args.val_cond))
    if args.out:
        print(f"last checkpoint: {ws.last_checkpoint}")
    return ws, history


def _dig(cfg: dict, keys, default=None):
    o = cfg
    for k in keys:
        if not isinstance(o, dict) or k not in o or o[k] is None:
            return default
        o = o[k]
    return o


if __name__ == "__main__":
    main()
