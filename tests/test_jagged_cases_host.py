"""CPU: every generator of tests/_jagged_cases.py has the property it is named for, by the rule
mirror _expected_kind of tests/test_gpu_sell.py -- so a failure of tests/test_gpu_jagged.py points at
a kernel and not at its input."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _jagged_cases as J
from tests.test_gpu_sell import _expected_kind


def _well_formed(A):
    A = sp.csr_matrix(A)
    assert A.has_canonical_format and np.all(A.data != 0)
    B = A.copy()
    B.sort_indices()
    assert np.array_equal(B.indices, A.indices)


def _kinds(A):
    """(kind with the default SELL-64X floor, kind with the floor lowered to 0)"""
    return _expected_kind(A), _expected_kind(A, xs_min_n=0)


def _lens(A):
    return np.diff(A.indptr)


def test_generators_are_quick_and_seeded():
    t0 = time.perf_counter()
    A = J.sweep(1500)
    assert time.perf_counter() - t0 < 1.0
    B = J.sweep(1500)
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert np.array_equal(A.data, B.data)


def test_sweep_has_every_group_count_lane_and_full_slice():
    A = J.sweep(1500)
    _well_formed(A)
    assert A.shape == (4133, 4133) and 4133 == 64 * 64 + 37
    lens = _lens(A)
    assert np.array_equal(lens, J.sweep_lengths())
    assert lens.max() == 64
    full = lens[:4096].reshape(64, 64)
    lanes = set()
    for s in range(64):
        assert full[s].max() == s % 64 + 1
        if s % 8 == 0:
            assert np.all(full[s] == full[s, 0])
        else:
            assert full[s, (7 * s) % 64] == full[s].max() and full[s].min() == 0
            lanes.add((7 * s) % 64)
    assert len(lanes - {0}) >= 8  # the longest row on lanes other than 0
    cnt = J.group_counts(A)  # [slices, 16]
    groups = (cnt > 0).sum(axis=1)  # 4-entry groups of each slice's longest row
    assert set(groups) == set(range(1, 17))  # every group count 1..16: every residue mod the batch of 2
    assert np.any(cnt == 64)  # a slice whose 64 rows all reach one group
    assert np.any(cnt[:, 15] > 0)  # the register's last byte is in use
    assert lens[-1] == lens[4096:].max() == 23  # the tail slice's longest row is the matrix's last
    rows = np.repeat(np.arange(4133), lens)
    assert np.all(np.abs(A.indices - rows) <= 1500)
    slots = 256.0 * ((np.pad(lens, (0, 27)).reshape(65, 64).max(axis=1) + 3) // 4).sum()
    assert 1.15 < slots / A.nnz <= 2.0
    assert J.tile_blocks(A).max() <= J.XMAX
    assert _kinds(A) == (17, 18)


def test_sweep_2200_keeps_a_tile_over_the_limit():
    A = J.sweep(2200)
    _well_formed(A)
    assert J.tile_blocks(A).max() > J.XMAX
    assert np.array_equal(_lens(A), J.sweep_lengths())
    assert _kinds(A) == (17, 17)


def test_limit_pair_is_exactly_256_and_257_blocks():
    A, B = J.limit(256), J.limit(257)
    for M in (A, B):
        _well_formed(M)
        assert M.shape[0] >= 4112 and _lens(M).max() <= 64
    ta, tb = J.tile_blocks(A), J.tile_blocks(B)
    assert ta[0] == ta.max() == 256 and tb[0] == tb.max() == 257
    assert np.array_equal(ta[1:], tb[1:]) and ta[1:].max() < 100
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.data, B.data)
    diff = np.flatnonzero(A.indices != B.indices)
    assert diff.size == 1 and (A.indices[diff[0]], B.indices[diff[0]]) == (4095, 4101)
    assert _kinds(A) == (17, 18) and _kinds(B) == (17, 17)


def test_row65_does_not_go_jagged():
    A, S = J.row65(), J.sweep(1500)
    _well_formed(A)
    assert _lens(A).max() == 65 and A.nnz == S.nnz + 1
    assert np.count_nonzero(_lens(A) != _lens(S)) == 1
    k = _kinds(A)
    assert k[0] == k[1] and k[0] in (0, 16)


@pytest.mark.parametrize("n", J.SIZES)
def test_sizes_are_ragged_and_jagged(n):
    A = J.sizes(n)
    _well_formed(A)
    lens = _lens(A)
    assert A.shape == (n, n) and lens.min() == 0 and lens.max() == 20 and lens[-1] == 17
    rows = np.repeat(np.arange(n), lens)
    per_slice = [np.unique((A.indices - rows)[rows // 64 == s]).size for s in range((n + 63) // 64)]
    assert min(per_slice) > 16  # no SELL-DIA
    assert _kinds(A) == (17, 18)
    assert {m % 256 for m in J.SIZES} >= {0, 1, 255} and 63 in J.SIZES and 64 in J.SIZES  # below one tile, n = 0, 1, 255 mod 256


@pytest.mark.parametrize("variant", ["last", "boundary"])
def test_holes(variant):
    A = J.holes(variant)
    _well_formed(A)
    n = A.shape[0]
    lens = _lens(A)
    assert n % 16 != 0 and n % 256 == 76
    assert lens[256:512].sum() == 0 and lens[576:640].sum() == 0  # a tile / a slice without entries
    assert lens[512:576].sum() > 0 and lens[640:768].sum() > 0  # ... the slice inside a live tile
    tb = J.tile_blocks(A)
    assert tb[1] == 0 and tb[[0, 2, 3, 4]].min() > 0
    if variant == "last":
        assert A.indices.max() == n - 1
    else:
        assert A.indices.max() == 639 and (A.indices.max() + 1) % 16 == 0 and A.indices.max() + 1 < n - 256
    assert _kinds(A) == (17, 18)


def test_off16_at_the_16_bit_limit():
    A, B = J.off16(32767), J.off16(32768)
    for M in (A, B):
        _well_formed(M)
        assert M.shape == (40000, 40000)
    rows = np.repeat(np.arange(40000), _lens(A))
    off = A.indices - (rows // 64) * 64
    assert off.max() == 32767 and off.min() == -32767
    rows = np.repeat(np.arange(40000), _lens(B))
    off = B.indices - (rows // 64) * 64
    assert off.max() == 32768 and off.min() == -32767
    assert _kinds(A) == (17, 18)
    k = _kinds(B)
    assert k[0] == k[1] and k[0] in (0, 32)


@pytest.mark.parametrize("exact32", [True, False])
@pytest.mark.parametrize("n", [4500, 4353])
def test_hub_spd(n, exact32):
    A = J.hub_spd(n, exact32)
    _well_formed(A)
    assert A.shape == (n, n) and n > 3072
    assert (abs(A - A.T)).nnz == 0  # symmetric, bit for bit
    d = A.diagonal()
    offsum = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert np.all(d > offsum)  # strictly diagonally dominant with a positive diagonal: SPD
    lens = _lens(A)
    assert [int(lens[h]) for h in J.hub_rows(n)] == list(J.HUB_TARGETS)
    assert lens.max() == 64 and np.count_nonzero(lens > 60) == 4
    assert [h % 64 for h in J.hub_rows(n)] == [1, 22, 43, 63]
    assert np.diff(J.hub_rows(n)).min() > 600  # no row couples to two hubs
    f32 = np.all(A.data.astype(np.float32).astype(np.float64) == A.data)
    assert f32 == exact32
    if not exact32:
        assert np.mean(A.data.astype(np.float32).astype(np.float64) != A.data) > 0.9
    assert _kinds(A) == (17, 18)


def test_banded_spd_is_what_the_tile_walk_needs():
    A = J.banded_spd(20000, 1500, seed=1)
    _well_formed(A)
    assert (abs(A - A.T)).nnz == 0
    d = A.diagonal()
    assert np.all(d > np.asarray(abs(A).sum(axis=1)).ravel() - d)
    assert J.tile_blocks(A).max() <= J.XMAX and _lens(A).max() <= 64
    assert _kinds(A) == (17, 18)
    assert np.all(A.data.astype(np.float32).astype(np.float64) == A.data)
