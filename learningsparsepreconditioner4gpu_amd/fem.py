"""P1 heat and elasticity operators of a tetrahedral mesh, assembled on the device.

``TetMesh`` is the device form of what the reference computes with ``pymathprim.geometry`` --
``laplacian(nodes, elem) + diags(lumped_mass(...) * field)`` (``datagen/heat_tetmesh.py:17-56``,
``datagen/heat.py``) and the block stiffness of ``datagen/elast_twist.py`` -- and of this package's
numpy stand-ins ``problems.p1_stiffness``, ``lumped_mass``, ``p1_laplacian_exact`` and the block
stiffness inside ``elasticity_box``.  The analysis (pattern and gather map, ``lspcg_fem_create``) runs
once per connectivity; every assembly after it writes the values of a live ``DeviceMatrix`` in place,
so mesh + coefficients -> A -> sample -> GNN -> L -> PCG runs without a host round trip::

    mesh = fem.TetMesh(nodes, tets)
    A = mesh.heat(kappa0, rho); live = ws.live_solver(A, mask, feats)
    for k in steps: mesh.heat(kappa_k, rho, out=A); live.refresh(); live.solve(b, x)

The arithmetic is fixed (``include/lspcg.h``): the expressions of ``problems.p1_laplacian_exact`` per
tet in double, each stored value the left-to-right sum of its contributions in ascending tet order,
the mass term of a diagonal entry last, one rounding to the matrix dtype.  The result is symmetric
bit for bit and does not depend on the launch.

A per-vertex coefficient becomes the per-tet one the operators take by ``field[tets].mean(1)``
(the reference's ``to_tet_field``, ``heat.py:15-19``); it is one torch expression, not a kernel here.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .sparse import Context, DeviceMatrix, _ptr

_I32_MAX = 2 ** 31 - 1


def _as_tensor(a, name: str) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.flags.writeable else a.copy())  # (torch refuses read-only memory)
    raise TypeError(f"{name} must be a numpy array or a torch tensor, got {type(a).__name__}")


class TetMesh:
    """A tet mesh on the device: ``nodes [N,3]`` float64 and ``tets [T,4]`` int32 or int64 (narrowed
    after a range check), numpy arrays or tensors on the host or on ``ctx``'s device.

    A vertex index outside ``0..N-1``, a tet that repeats a vertex and a tet of zero or non-finite
    determinant raise ``LspcgError`` (``ERR_FORMAT``, naming the first such tet).  Either orientation
    of a tet is accepted.  Calls on one mesh run on one stream at a time."""

    def __init__(self, nodes, tets, ctx: Optional[Context] = None):
        nodes = self._check_nodes(nodes, None)
        tets = _as_tensor(tets, "tets")
        if tets.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"tets is {tets.dtype}, expected int32 or int64")
        if tets.ndim != 2 or tets.shape[1] != 4:
            raise ValueError(f"tets has shape {tuple(tets.shape)}, expected (T, 4)")
        if tets.dtype == torch.int64 and tets.numel() and \
                (int(tets.min()) < -_I32_MAX - 1 or int(tets.max()) > _I32_MAX):
            raise ValueError("tets holds an index outside the int32 range")
        self.ctx = ctx if ctx is not None else Context.get(nodes.device if nodes.is_cuda else None)
        dev = self.ctx.torch_device
        for name, a in (("nodes", nodes), ("tets", tets)):
            if a.device.type != "cpu" and a.device != dev:
                raise ValueError(f"{name} is on {a.device}, the context is on {dev}")
        nodes = nodes.contiguous()
        tets = tets.to(torch.int32).contiguous()
        self.handle = None
        h = C.c_void_p()
        _lib.call("lspcg_fem_create", self.ctx.handle, nodes.shape[0], tets.shape[0], _ptr(nodes), _ptr(tets),
                  C.byref(h))
        self.handle = h
        n, t, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.call("lspcg_fem_info", h, C.byref(n), C.byref(t), C.byref(nnz))
        self.num_nodes, self.num_tets, self.nnz = n.value, t.value, nnz.value

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value and _lib._lib is not None:
            _lib._lib.lspcg_fem_destroy(h)
            self.handle = None

    # ---- argument checks (all before any native call)
    @staticmethod
    def _check_nodes(nodes, n: Optional[int]) -> torch.Tensor:
        nodes = _as_tensor(nodes, "nodes")
        if nodes.dtype != torch.float64:
            raise TypeError(f"nodes is {nodes.dtype}, expected torch.float64")
        if nodes.ndim != 2 or nodes.shape[1] != 3 or (n is not None and nodes.shape[0] != n):
            raise ValueError(f"nodes has shape {tuple(nodes.shape)}, expected ({'N' if n is None else n}, 3)")
        return nodes

    def _field(self, v, count: int, name: str, scalar_ok: bool):
        """A coefficient as (device fp64 tensor of ``count`` entries | None, float): a Python / numpy
        scalar stays a scalar (``scalar_ok``) or is broadcast."""
        if isinstance(v, (bool, str)) or v is None:
            raise TypeError(f"{name} must be a number, a numpy array or a tensor, got {type(v).__name__}")
        if isinstance(v, (int, float, np.integer, np.floating)):
            if scalar_ok:
                return None, float(v)
            return torch.full((count,), float(v), dtype=torch.float64, device=self.ctx.torch_device), 0.0
        t = _as_tensor(v, name)
        if t.dtype != torch.float64:
            raise TypeError(f"{name} is {t.dtype}, expected torch.float64")
        if t.ndim != 1 or t.shape[0] != count:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected ({count},)")
        if t.device.type != "cpu" and t.device != self.ctx.torch_device:
            raise ValueError(f"{name} is on {t.device}, the mesh is on {self.ctx.torch_device}")
        return t.to(self.ctx.torch_device).contiguous(), 0.0

    def _out(self, out) -> Optional[DeviceMatrix]:
        if out is None:
            return None
        if not isinstance(out, DeviceMatrix):
            raise TypeError(f"out must be a DeviceMatrix, got {type(out).__name__}")
        if out.ctx is not self.ctx:
            raise ValueError("out belongs to another context")
        return out  # its size, block size and pattern are compared natively (ERR_FORMAT, nothing written)

    # ---- the pattern
    def pattern(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(indptr [N+1], indices [nnz])``, int32 on the device: sorted columns, every diagonal stored."""
        dev = self.ctx.torch_device
        indptr = torch.empty(self.num_nodes + 1, dtype=torch.int32, device=dev)
        indices = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        _lib.call("lspcg_fem_pattern", self.handle, _ptr(indptr), _ptr(indices))
        return indptr, indices

    def matrix(self, dtype=torch.float64, block_size: int = 1) -> DeviceMatrix:
        """A ``DeviceMatrix`` on the mesh's pattern with all values 0 (scalar, or 3x3 blocks)."""
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"unsupported dtype {dtype} (torch.float32 / torch.float64 only)")
        if block_size not in (1, 3):
            raise ValueError(f"block_size is {block_size}, expected 1 or 3")
        indptr, indices = self.pattern()
        vals = torch.zeros(self.nnz * block_size * block_size, dtype=dtype, device=self.ctx.torch_device)
        return DeviceMatrix.from_device_csr(indptr, indices, vals, self.num_nodes * block_size, block_size=block_size,
                                            ctx=self.ctx)

    # ---- the operators
    def lumped_mass(self) -> torch.Tensor:
        """``m_i = Σ vol_t / 4`` over the tets of vertex i: ``[N]`` float64 on the device."""
        m = torch.empty(self.num_nodes, dtype=torch.float64, device=self.ctx.torch_device)
        _lib.call("lspcg_fem_lumped_mass", self.handle, _ptr(m))
        return m

    def heat(self, kappa=None, density=0.0, out: Optional[DeviceMatrix] = None) -> DeviceMatrix:
        """``A = K(kappa) + diag(density ⊙ lumped_mass)``.  ``kappa``: ``[T]`` float64 per tet, a
        number, or None (1); ``density``: a number or ``[N]`` float64 per vertex.  ``out``: a scalar
        matrix on the mesh's pattern (``mesh.matrix()``, or an earlier result) overwritten in place
        as by ``set_values`` -- a solver on it needs ``update_matrix()`` before its next solve;
        another pattern, size or block size raises ``LspcgError`` (``ERR_FORMAT``) and writes nothing.
        ``out=None`` allocates a float64 ``mesh.matrix()``."""
        kap = None if kappa is None else self._field(kappa, self.num_tets, "kappa", scalar_ok=False)[0]
        rho, rho_scalar = self._field(density, self.num_nodes, "density", scalar_ok=True)
        out = self._out(out)
        if out is None:
            out = self.matrix()
        _lib.call("lspcg_fem_heat", self.handle, _ptr(kap) if kap is not None else None,
                  _ptr(rho) if rho is not None else None, rho_scalar, out.handle)
        out.values_version += 1
        return out

    def laplacian(self, kappa=None, out: Optional[DeviceMatrix] = None) -> DeviceMatrix:
        """The P1 stiffness ``K(kappa)``: :meth:`heat` with density 0."""
        return self.heat(kappa, 0.0, out=out)

    def elasticity(self, young, poisson, mass_coef: float = 0.0, out: Optional[DeviceMatrix] = None) -> DeviceMatrix:
        """The linear-elastic P1 stiffness in 3x3 blocks plus ``mass_coef · lumped_mass`` on the
        diagonal (``problems.elasticity_box``'s operator; there ``mass_coef = density / dt²``).
        ``young`` / ``poisson``: a number or ``[T]`` float64 per tet.  ``out``: a block-size-3 matrix
        on the mesh's pattern, as for :meth:`heat`; ``out=None`` allocates ``mesh.matrix(block_size=3)``."""
        E = self._field(young, self.num_tets, "young", scalar_ok=False)[0]
        nu = self._field(poisson, self.num_tets, "poisson", scalar_ok=False)[0]
        if isinstance(mass_coef, (bool, str)) or not isinstance(mass_coef, (int, float, np.integer, np.floating)):
            raise TypeError(f"mass_coef must be a number, got {type(mass_coef).__name__}")
        out = self._out(out)
        if out is None:
            out = self.matrix(block_size=3)
        _lib.call("lspcg_fem_elasticity", self.handle, _ptr(E), _ptr(nu), float(mass_coef), out.handle)
        out.values_version += 1
        return out

    def set_nodes(self, nodes) -> "TetMesh":
        """Moved vertices on the same connectivity.  A tet that became flat raises ``LspcgError``
        (``ERR_FORMAT``) and the old coordinates stay."""
        nodes = self._check_nodes(nodes, self.num_nodes)
        if nodes.device.type != "cpu" and nodes.device != self.ctx.torch_device:
            raise ValueError(f"nodes is on {nodes.device}, the mesh is on {self.ctx.torch_device}")
        nodes = nodes.contiguous()
        _lib.call("lspcg_fem_set_nodes", self.handle, _ptr(nodes))
        return self
