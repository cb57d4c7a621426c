"""The multi-row GEMMs kernel by kernel (k_mgemm<1,1>, <2,1>, <4,1>, <4,2>,
<4,4>, k_pgemm<2>, k_pgemm<4>, their split forms through k_mgemm_reduce, and
k_split3) through the kernel-level entry qtts_hip_rows_gemm_case, against the
float64 reference and bound of rows_gemm_ref.py.

Every case: every output element within the bound (the exact-plane cases:
equal to the float64 result bit for bit, whatever the summation order or
split); the kernel and kz that ran are the ones the case was written for; the
x rows are longer than C with NaN behind them, so an over-read shows as a NaN;
the y rows are longer than the output, there are rows behind the last one, and
everything outside the written pattern comes back bit-identical; the split
workspace, the plane scratch and the 1/rms scratch are allocated larger than
stated and the tail comes back untouched.  The cases are rows_gemm_cases.py's;
test_rows_gemm_ref.py checks on the same inputs that the check would notice a
wrong kernel.
"""
import numpy as np
import pytest

import qtts
import rows_gemm_ref as G
from rows_gemm_cases import AUTO, CASES, EXACT, REFUSED, describe

pytestmark = pytest.mark.gpu

_RATIO = {}   # kernel (and split form) -> largest err / bound, printed for DESIGN.md
_SEEN = {}    # kernel -> largest kz reported by a passing case
PLANE_SENTINEL = 0x7FC1   # a bf16 NaN: a plane element read from the tail poisons the output


def _dev(a, gpu):
    import torch
    a = np.array(a)   # (a copy: the shared reference inputs are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def run_case(gpu, cs, d, **over):
    """runs the case; returns (the plan that ran or None, y after, y before)"""
    import torch
    keep, ptr = {}, {}

    def put(name, a):
        keep[name] = _dev(a, gpu)
        ptr[name] = keep[name].data_ptr()

    put("A", d["W"])
    if cs.src == "x":
        ldx = over.get("ldx") or cs.C + G.PAD_X
        x = np.full(cs.M * ldx + 8, np.nan, np.float32)   # (+ 8: room for the misaligned case's shifted rows)
        off = over.get("x_off", 0) // 4
        for m in range(cs.M):
            x[off + m * ldx:off + m * ldx + cs.C] = d["x"][m]
        put("x", x)
    else:
        put("table", d["table"])
        put("ids", d["ids"])
    for k in ("norm_w", "bias"):
        if k in d:
            put(k, d[k])
    y0 = G.y_buffer(cs, d)
    put("y", y0)
    put("part", np.full(cs.part + G.TAIL, G.SENTINEL, np.float32))
    put("planes", np.full(cs.plane_elems + G.TAIL, PLANE_SENTINEL, np.uint16))
    put("inv", np.full(cs.M + G.TAIL, G.SENTINEL, np.float32))
    ran = qtts.Kernels.rows_gemm_case(describe(cs, ptr, **over), cs.force)
    torch.cuda.synchronize()
    part, pl, inv = keep["part"].cpu().numpy(), keep["planes"].cpu().numpy().view(np.uint16), keep["inv"].cpu().numpy()
    assert np.all(part[cs.part:].view(np.uint32) == G.SENTINEL.view(np.uint32)), "wrote behind the split workspace"
    assert np.all(pl[cs.plane_elems:] == PLANE_SENTINEL), "wrote behind the plane scratch"
    assert np.all(inv[cs.M:].view(np.uint32) == G.SENTINEL.view(np.uint32)), "wrote behind the 1/rms scratch"
    if ran is not None and ran["kz"] > 1:     # the partials beyond kz M R are not the kernel's either
        used = ran["kz"] * cs.M * cs.R
        assert np.all(part[used:].view(np.uint32) == G.SENTINEL.view(np.uint32)), "wrote behind kz M R partials"
    return ran, keep["y"].cpu().numpy(), y0


def check_case(gpu, cs, keep=True):
    d, ref, bound = G.reference(cs, keep=keep)
    ran, y, y0 = run_case(gpu, cs, d)
    assert ran is not None, ("not covered", cs.id())
    assert (ran["kernel"], ran["kz"]) == (cs.kernel, cs.kz), (ran, cs.id())
    ok, ratio, why = G.check(cs, y, y0, ref, bound)
    name = cs.kernel + (" split" if cs.kz > 1 else "") + (" exact" if cs.exact else "")
    print(f"{'differing' if cs.exact else 'err / bound'}  {name:24s} {ratio:.4f}  {cs.id()}")
    if not ok and cs.exact:                   # the pattern of differing elements, for the record
        bad = np.argwhere(y[:cs.M, :cs.nout].astype(np.float64) != ref)
        print("differing (row, output):", bad[:16].tolist(), "rows", sorted(set(bad[:, 0].tolist()))[:16])
    assert ok, (cs.id(), why, ratio)
    if not cs.exact:
        _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    _SEEN[cs.kernel] = max(_SEEN.get(cs.kernel, 0), cs.kz)


@pytest.mark.parametrize("cs", CASES, ids=[cs.id() for cs in CASES])
def test_case(gpu, cs):
    check_case(gpu, cs)


@pytest.mark.parametrize("cs", EXACT, ids=[cs.id() for cs in EXACT])
def test_exact_planes(gpu, cs):
    """inputs whose three planes are known and whose partial sums are all exact
    in fp32: a lost, misrouted or double-counted plane, stage or split column
    changes the result, and any change is a failure"""
    check_case(gpu, cs)


@pytest.mark.parametrize("cs", AUTO, ids=[cs.id() for cs in AUTO])
def test_prefill_dispatch_runs_what_rows_proj_takes(gpu, cs, monkeypatch):
    """force -1: the launcher and kernel of the runtime's prefill dispatch --
    k_pgemm on the two shipped shapes, k_mgemm where k_pgemm does not cover"""
    monkeypatch.delenv("QTTS_HIP_PGEMM_BN", raising=False)
    check_case(gpu, cs, keep=False)


@pytest.mark.parametrize("what,cs,over", REFUSED, ids=[r[0] for r in REFUSED])
def test_forced_pgemm_launches_nothing_on_what_it_does_not_cover(gpu, what, cs, over):
    d = G.make_inputs(cs)
    ran, y, y0 = run_case(gpu, cs, d, **over)
    assert ran is None, what
    assert np.array_equal(y.view(np.uint32), y0.view(np.uint32)), what


def test_zz_every_kernel_and_both_reduces_ran(gpu):
    """from the reports of the cases above (runs last in this module): each of
    the seven kernels ran, and each ran with kz > 1 (k_mgemm's and k_pgemm's
    partials through k_mgemm_reduce)"""
    for k in qtts.RG_NAMES:     # (run on its own, or out of order: the first split case of the kernel)
        if _SEEN.get(k, 0) <= 1:
            check_case(gpu, next(cs for cs in CASES + EXACT if cs.kernel == k and cs.kz > 1))
    for k in sorted(_RATIO):
        print(f"err / bound  {k:32s} {_RATIO[k]:.4f}")
    assert sorted(_SEEN) == sorted(qtts.RG_NAMES), _SEEN
    assert all(v > 1 for v in _SEEN.values()), _SEEN
