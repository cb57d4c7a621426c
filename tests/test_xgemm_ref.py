"""The codec contraction tests' float64 bound and the dispatcher's planner,
checked without a device on the inputs test_gpu_xgemm.py runs.

(a) On the plane-planted inputs the bound tells each of the five lower
    bf16-plane products from the right answer at every element (by >= 2x) while
    a sequential fp32 accumulation stays below half of it.
(b) On the random inputs, every listed mutation of the reference exceeds the
    bound on at least one element (test_gpu_xgemm.py fails on any single
    exceedance).
(c) The planner (qtts_hip_xgemm_plan, host only) reports the kernel and split
    count every case was written for, refuses forced kernels on shapes they
    do not cover, and keeps its choices for the shipped 1.7B decode shapes.
"""
import numpy as np
import pytest

import qtts
import xgemm_ref as X
from xgemm_cases import CASES, REFUSED, SHIPPED, describe, fake_ptrs, shipped

PLANTED = [sp for sp in CASES if sp.planted]
RANDOM = [sp for sp in CASES if not sp.planted and sp.M * sp.N * sp.kdim <= 1 << 24]


def _ids(cases):
    return [sp.id() for sp in cases]


# ------------------------------------------------------------------ (a)
def test_planted_cases_cover_the_three_plane_kernels():
    paths = {sp.path for sp in PLANTED}
    assert paths == {X.XP_CONVB2, X.XP_CONVB4, X.XP_XLIN}
    assert any(sp.kind == "tconv" for sp in PLANTED)


@pytest.mark.parametrize("sp", PLANTED, ids=_ids(PLANTED))
def test_bound_tells_every_dropped_plane_product(sp):
    d, _, _ = X.reference(sp)
    _, b_acc = X.accumulate(sp, d)
    for ph in range(sp.stride):
        A, B = X.operands(sp, d, ph)
        assert np.count_nonzero(A[0]) <= 112
        bound = b_acc[:, ph::sp.stride]
        ref = A.astype(np.float64) @ B.astype(np.float64)
        ap, bp = X.planes(A), X.planes(B)
        assert np.array_equal(sum(ap), A.astype(np.float64)) and np.array_equal(sum(bp), B.astype(np.float64))
        nz = np.abs(ref) > 0          # (columns whose taps all fall left of tmin hold no product)
        assert nz.all()
        full = sum(ap[i] @ bp[j] for i, j in X.KEPT)
        assert np.all(np.abs(full - ref) <= 0.1 * bound)
        for drop in X.KEPT[1:]:
            got = sum(ap[i] @ bp[j] for i, j in X.KEPT if (i, j) != drop)
            assert np.all(np.abs(got - ref)[nz] >= 2 * bound[nz]), drop
        acc = np.zeros(ref.shape, np.float32)     # float32, sequential over k
        for k in range(A.shape[1]):
            acc = (acc + np.outer(A[:, k], B[k]).astype(np.float32)).astype(np.float32)
        assert np.all(np.abs(acc - ref) <= 0.5 * bound)


# ------------------------------------------------------------------ (b)
def _out(sp, d, kw=None, bias_swap=False, **mut):
    acc, b_acc = X.accumulate(sp, d, kw=kw, **mut)
    return X.epilogue(sp, d, acc, b_acc, bias_swap=bias_swap)[0]


def _stage(sp):
    """K columns of the kernel's last channel / K stage"""
    if sp.kind != "lin":
        return min(16, sp.ci) * sp.ntap
    return 128 if sp.path == X.XP_XLIN else 32


def _prefill(sp, d, ref):
    """what C holds before the call, in the logical layout"""
    c0 = d.get("c0")
    if c0 is None:
        return np.full(ref.shape, float(X.SENTINEL))
    return (c0.T if sp.emode in X.T_MODES else c0).astype(np.float64)


def mutants(sp, d, ref):
    """[(name, output)] of every mutation that applies to the case"""
    K, out = sp.kdim, []
    conv, tc = sp.kind == "conv", sp.kind == "tconv"
    if conv or tc:
        out.append(("tap 0 shifted by -1", _out(sp, d, tap_shift=(0, -1))))
        if sp.ntap > 1:
            out.append(("last tap shifted by -1", _out(sp, d, tap_shift=(sp.ntap - 1, -1))))
        out.append(("tmin + 1", _out(sp, d, dtmin=1)))
        if sp.halo > 0 and not sp.hist:      # (with the whole halo as history no tap reaches tmin - 1)
            out.append(("tmin - 1", _out(sp, d, dtmin=-1)))
    if conv:
        if sp.Kw > 1:
            out.append(("dilation + 1", _out(sp, d, ddil=1)))
            out.append(("dilation - 1", _out(sp, d, ddil=-1)))
        out.append(("left pad + 1", _out(sp, d, dpad=1)))
        if sp.N > 1:
            out.append(("left pad - 1", _out(sp, d, dpad=-1)))
    kw = np.ones(K)
    kw[K - _stage(sp):] = 0.0
    if sp.kind == "lin" and K % _stage(sp):
        kw = np.ones(K)
        kw[K - K % _stage(sp):] = 0.0
    out.append(("last stage dropped", _out(sp, d, kw=kw)))
    rng = X.split_ranges(sp) if sp.splits > 1 else None
    if rng:
        for z in {0, len(rng) - 1}:
            for f, name in ((0.0, "dropped"), (2.0, "counted twice")):
                kw = np.ones(K)
                kw[rng[z][0]:rng[z][1]] = f
                out.append((f"split {z} {name}", _out(sp, d, kw=kw)))
    if tc and sp.stride > 1:
        m = ref.copy()
        m[:, 0::sp.stride], m[:, 1::sp.stride] = ref[:, 1::sp.stride], ref[:, 0::sp.stride]
        out.append(("phases 0 and 1 swapped", m))
    if sp.snake:
        out.append(("neighbour's SnakeBeta parameters", _out(sp, d, snake_roll=1)))
    if "bias" in d and min(sp.M, sp.N) > 1:
        out.append(("bias[m] <-> bias[n]", _out(sp, d, bias_swap=True)))
    pre = _prefill(sp, d, ref)
    m = ref.copy()
    m[:, -1] = pre[:, -1]
    out.append(("last column missing", m))
    m = ref.copy()
    m[-1] = pre[-1]
    out.append(("last row missing", m))
    return out


@pytest.mark.parametrize("sp", RANDOM, ids=_ids(RANDOM))
def test_bound_notices_a_wrong_reference(sp):
    d, ref, bound = X.reference(sp)
    assert np.all(np.isfinite(ref)) and np.all(bound > 0)
    for name, got in mutants(sp, d, ref):
        if np.array_equal(got, ref):
            continue      # not a mutant here: the case never reads what it changes (one column, no history)
        assert np.any(np.abs(got - ref) > bound), name


def test_every_mutation_is_exercised():
    want = {"tap 0 shifted by -1", "last tap shifted by -1", "tmin + 1", "tmin - 1", "dilation + 1", "dilation - 1",
            "left pad + 1", "left pad - 1", "last stage dropped", "split 0 dropped", "split 0 counted twice",
            "phases 0 and 1 swapped", "neighbour's SnakeBeta parameters", "bias[m] <-> bias[n]",
            "last column missing", "last row missing"}
    seen = {}
    for sp in RANDOM:
        if sp.M * sp.N * sp.kdim <= 1 << 21:
            d, ref, _ = X.reference(sp)
            for n, got in mutants(sp, d, ref):
                seen[n] = seen.get(n, 0) + (not np.array_equal(got, ref))
    assert all(seen.get(n, 0) >= 3 for n in want), {n: seen.get(n, 0) for n in want}


# ------------------------------------------------------------------ (c)
def _plan(sp, force=None):
    return qtts.Kernels.xgemm_plan(describe(sp, fake_ptrs(sp)), sp.part, sp.force if force is None else force)


@pytest.mark.parametrize("sp", CASES, ids=_ids(CASES))
def test_planner_reports_what_the_case_was_written_for(sp):
    assert _plan(sp) == (sp.path, sp.splits)


@pytest.mark.parametrize("sp", REFUSED, ids=_ids(REFUSED))
def test_forced_kernel_refuses_a_shape_it_does_not_cover(sp):
    assert _plan(sp) is None


def test_cases_reach_every_kernel_and_both_reduces():
    seen = {}
    for sp in CASES:
        seen[sp.path] = max(seen.get(sp.path, 0), sp.splits)
    assert sorted(seen) == list(range(6))
    assert all(v > 1 for v in seen.values())


@pytest.mark.parametrize("T", [1, 16, 128])
def test_planner_keeps_the_shipped_choices(T):
    got = [(name,) + _plan(sp, -1) for name, sp in shipped(T)]
    assert got == SHIPPED[T]
    # no shipped shape reaches the fp32 conv kernel: SnakeBeta never covers more than 1536 channels per split
    assert all(p != X.XP_CONV for _, p, _ in got)
