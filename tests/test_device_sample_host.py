"""Host side of "the GNN's input sample built on the device": the two calls are declared, bound and
exported, the codes match the header, the host path of make_sample is what it was, and the device
entry points check their options before any native call and fail loudly without a GPU (no GPU here)."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from learningsparsepreconditioner4gpu_amd import _build, _lib, data, workspace
from learningsparsepreconditioner4gpu_amd import problems as P
from learningsparsepreconditioner4gpu_amd.dataset import RawData, make_data

ROOT = Path(__file__).resolve().parents[1]
NEW = {"lspcg_mat_edge_index": 2, "lspcg_mat_sample": 12}


def _header():
    return (ROOT / "include" / "lspcg.h").read_text()


def test_the_two_calls_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs, name
    assert _lib.SIGNATURES["lspcg_mat_sample"][1][2]._type_ is _lib.lspcg_sample_desc
    assert "lspcg_sample.hip" in _build.SOURCES
    if not _lib.LIB_PATH.exists():
        pytest.fail(f"{_lib.LIB_PATH} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (lspcg_[a-z0-9_]+)$", out.stdout, flags=re.M))
    assert set(NEW) <= exported, set(NEW) - exported


def test_the_codes_match_the_header():
    defs = dict(re.findall(r"#define (LSPCG_(?:NORM|REDUCE)_[A-Z0-9]+) (\d+)", _header()))
    assert {k[len("LSPCG_NORM_"):].lower(): int(v) for k, v in defs.items() if k.startswith("LSPCG_NORM_")} == _lib.NORM
    assert ({k[len("LSPCG_REDUCE_"):].lower(): int(v) for k, v in defs.items() if k.startswith("LSPCG_REDUCE_")}
            == _lib.REDUCE)
    assert len(_lib.NORM) == 4 and len(_lib.REDUCE) == 5
    m = re.search(r"typedef struct lspcg_sample_desc \{(.*?)\} lspcg_sample_desc;", _header(), flags=re.S)
    fields = re.findall(r"\bint (\w+);", m.group(1))
    assert fields == [n for n, _ in _lib.lspcg_sample_desc._fields_]


def test_make_sample_of_a_scipy_matrix_is_unchanged():
    """The host path still goes through dataset.make_data: the same field types and the same values."""
    A, mask, _ = P.poisson2d_grid(5, 4)
    A = sp.csr_matrix(A)
    rng = np.random.default_rng(0)
    nf = rng.standard_normal((A.shape[0], 2))
    got = data.make_sample(A, mask=mask, node_features=nf, use_edge_features_as_node_feature="sum",
                           normalize_matrix="frob")
    g = P.to_block_graph(A, 1)
    raw = RawData(block_values=g.block_values, diagonals=A.diagonal().reshape(-1, 1), edge_index=g.edge_index,
                  node_features=nf, lhs=None, rhs=None, mask=np.asarray(mask, dtype=np.float64).reshape(-1, 1),
                  num_nodes=g.num_nodes, block_size=1)
    want = make_data(raw, use_edge_features_as_node_feature="sum", normalize_matrix="frob")
    assert isinstance(got, data.GraphSample)
    assert got.matrix_scale == want.matrix_scale == 1.0 / np.linalg.norm(g.block_values)
    assert got.block_size == 1 and got.x.shape == (20, 2 + 1 + 1)
    for name in ("x", "edge_index", "edge_attr", "mask", "matrix_values", "diagonal", "inv_diag", "rsqrt_diag", "ptr"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.device.type == "cpu" and a.dtype == b.dtype and torch.equal(a, b), name
    assert got.residual is None and got.gt is None


def test_the_python_entry_points_exist():
    p = inspect.signature(data.DeviceSampler.__init__).parameters
    assert list(p)[:4] == ["self", "A", "mask", "node_features"]
    for name in ("use_mask_as_node_feature", "use_edge_features_as_node_feature", "normalize_matrix", "is_inference"):
        assert p[name].default == inspect.signature(data.make_sample).parameters[name].default
    assert "use_node_features_as_edge_feature" not in p
    assert list(inspect.signature(data.DeviceSampler.sample).parameters) == ["self", "A", "node_features"]
    p = inspect.signature(workspace.SimpleInferenceWorkspace.live_solver).parameters
    assert list(p)[:5] == ["self", "A", "mask", "node_features", "dtype"] and p["dtype"].default is np.float64
    for name in ("refresh", "solve", "residual"):
        assert callable(getattr(workspace.LiveSolver, name))
    p = inspect.signature(workspace.LiveSolver.solve).parameters
    assert list(p)[:5] == ["self", "b", "x", "rtol", "max_iter"] and p["refine"].default > 0
    assert workspace.ScaledInferenceWorkspace.live_solver is workspace.SimpleInferenceWorkspace.live_solver


@pytest.mark.parametrize("kw, match", [
    (dict(normalize_matrix="max"), "normalize_matrix"),
    (dict(normalize_matrix=2), "normalize_matrix"),
    (dict(use_edge_features_as_node_feature="prod"), "use_edge_features_as_node_feature"),
    (dict(normalize_matrix="l1", block_size=3), "block_size 1 only"),
    (dict(block_size=2), "block_size"),
    (dict(use_mask_as_node_feature=False), "No node feature"),
])
def test_options_are_checked_before_any_native_call(kw, match, monkeypatch):
    """Raised by the option check itself: neither the library nor the GPU is touched."""
    def refuse(*a, **k):
        raise AssertionError("a native call was made before the options were checked")

    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "load", refuse)
    A = P.elasticity_box(3, 3, 3)[0] if kw.get("block_size") == 3 else P.kuhn_laplacian(3)
    with pytest.raises(ValueError, match=match):
        data.DeviceSampler(A, **kw)
    ws = workspace.SimpleInferenceWorkspace(1, 1, block_size=1, device="cpu")
    with pytest.raises(ValueError, match=match):
        ws.live_solver(A, **kw)


def test_the_device_entry_points_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    A = P.kuhn_laplacian(3)
    with pytest.raises(_lib.LspcgUnavailable):
        data.DeviceSampler(A)
    for cls in (workspace.SimpleInferenceWorkspace, workspace.ScaledInferenceWorkspace):
        ws = cls(1, 1, block_size=1, device="cpu")
        with pytest.raises(_lib.LspcgUnavailable):
            ws.live_solver(A)
