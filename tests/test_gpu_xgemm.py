"""Every kernel of the codec's contraction family (k_codec.hip: k_convb<Kw,2>,
k_convb<Kw,4>, k_conv<Kw>, k_xlin, k_xgemv, k_xgemm, and the split forms
through k_conv_reduce / k_xg_reduce) through the kernel-level entry
qtts_hip_xgemm_case, against the float64 reference and bound of xgemm_ref.py.

Every case: every output element within the bound; the kernel and split
count that ran are the ones the case was written for; the input is NaN outside
the columns [tmin, L) a conv may read and in every row's padding, so an
over-read shows as a NaN; the output rows are longer than the data and
prefilled with a sentinel, and everything outside the M x N (or strided
phase) pattern comes back bit-identical; the split workspace is exactly as
large as the case states.  The cases are xgemm_cases.py's; test_xgemm_ref.py
checks on the same inputs that the bound would notice a wrong kernel.
"""
import numpy as np
import pytest

import qtts
import xgemm_ref as X
from xgemm_cases import CASES, REFUSED, SHIPPED, describe, layout, shipped

pytestmark = pytest.mark.gpu

_RATIO = {}   # kernel (and split form) -> largest err / bound, printed for DESIGN.md
_SEEN = {}    # kernel -> largest split count reported by a passing case


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def run_case(gpu, sp, d=None):
    """runs the case; returns ((path, splits) or None, C after, C before)"""
    d = X.reference(sp)[0] if d is None else d
    lo = layout(sp)
    K, nan = sp.kdim, np.float32(np.nan)
    keep, ptr = [], {}

    def put(name, a, off=0):
        t = _dev(a.astype(np.float32), gpu)
        keep.append(t)
        ptr[name] = t.data_ptr() + 4 * off

    if sp.kind == "lin":
        if sp.amode == X.XA_ROWS:
            A = np.full((sp.M, lo["lda"]), nan)
            A[:, :K] = d["A"]
        else:
            A = np.full((K, lo["lda"]), nan)
            A[:, :sp.M] = d["A"].T
        W = np.full((sp.N, lo["ldb"]), nan)
        W[:, :K] = d["W"]
        put("A", A)
        put("B", W)
    else:
        x = d["x"].copy()
        x[:, :X.LM + sp.tmin] = nan
        x[:, X.LM + sp.N:] = nan
        put("A", d["w"])
        put("B", x, X.LM)
    for k in ("sa", "sb", "bias", "vec", "ea", "eb"):
        if k in d:
            put(k, d[k])
    if "aux" in d:
        aux = np.full((sp.M, lo["ldaux"]), nan)
        aux[:, :sp.N] = d["aux"]
        put("aux", aux)
    C0 = np.full((lo["crows"], lo["ldc"]), X.SENTINEL, np.float32)
    if "c0" in d:
        C0[:d["c0"].shape[0], :d["c0"].shape[1]] = d["c0"]
    put("C", C0)
    import torch
    ran = qtts.Kernels.xgemm_case(describe(sp, ptr), sp.part, sp.force)
    torch.cuda.synchronize()
    return ran, keep[-1].cpu().numpy(), C0


def check_case(gpu, sp, tag=None):
    d, ref, bound = X.reference(sp, keep=tag is None)
    ran, C, C0 = run_case(gpu, sp, d)
    assert ran == (sp.path, sp.splits), (ran, sp.id())
    if sp.emode in X.T_MODES:
        ref, bound = ref.T, bound.T
    R, Cn = ref.shape
    got = C[:R, :Cn].astype(np.float64)
    err = np.abs(got - ref)
    ratio = float(np.max(err / bound)) if np.all(np.isfinite(got)) else float("inf")
    name = (tag or qtts.XP_NAMES[sp.path]) + (" split" if sp.splits > 1 and sp.path != X.XP_XGEMV else "")
    name += " planted" if sp.planted else ""
    print(f"err / bound  {name:32s} {ratio:.4f}  {sp.id()}")
    assert np.all(err <= bound), (sp.id(), ratio, np.argwhere(~(err <= bound))[:4])
    # everything outside the written pattern is untouched, bit for bit
    mask = np.ones(C.shape, bool)
    mask[:R, :Cn] = False
    assert np.array_equal(C.view(np.uint32)[mask], C0.view(np.uint32)[mask]), sp.id()
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    _SEEN[sp.path] = max(_SEEN.get(sp.path, 0), sp.splits)


@pytest.mark.parametrize("sp", CASES, ids=[sp.id() for sp in CASES])
def test_case(gpu, sp):
    check_case(gpu, sp)


@pytest.mark.parametrize("sp", REFUSED, ids=[sp.id() for sp in REFUSED])
def test_forced_kernel_launches_nothing_on_a_shape_it_does_not_cover(gpu, sp):
    ran, C, C0 = run_case(gpu, sp)
    assert ran is None
    assert np.array_equal(C.view(np.uint32), C0.view(np.uint32))


_SHIPPED_RUNS = [(T, i) for T in (1, 16) for i in range(len(SHIPPED[T]))]


@pytest.mark.parametrize("T,i", _SHIPPED_RUNS, ids=[f"T{T}-{SHIPPED[T][i][0]}" for T, i in _SHIPPED_RUNS])
def test_shipped_shape_runs_the_pinned_plan(gpu, T, i):
    """each contraction of a 1.7B decode of T frames under the planner's own
    choice with the model's workspace: the pinned kernel and splits, and right"""
    from dataclasses import replace
    cases = shipped(T)
    assert [n for n, _ in cases] == [n for n, _, _ in SHIPPED[T]]
    (name, sp), (_, path, splits) = cases[i], SHIPPED[T][i]
    check_case(gpu, replace(sp, path=path, splits=splits), tag=f"1.7B T={T} " + qtts.XP_NAMES[path])


def _grid(lo, hi, n):
    return np.linspace(lo, hi, n, dtype=np.float64).astype(np.float32)


def test_device_functions(gpu):
    """the device functions behind the bound's constants, against float64:
    snake with the GEMMs' own sin^2 within d_snake over |x a| <= 8192 (nothing
    else compares sin2 with anything); expf (relative) and tanhf (absolute)
    within FUNC_ERR_MAX over the epilogue inputs' range (|silu argument| <= 16,
    |gelu's tanhf argument| <= 12), so that the epilogues' 2e-7 covers them"""
    import torch
    rng = np.random.default_rng(5)
    Cn, L = 64, 8192
    a = rng.uniform(0.05, 8.0, Cn).astype(np.float32)
    ib = (rng.uniform(0.1, 4.0, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(np.float32)
    x = (rng.uniform(-1.0, 1.0, (Cn, L)) * (8192.0 / a[:, None]) * rng.choice([1e-3, 1e-2, 0.1, 1.0], (Cn, L)))
    x = x.astype(np.float32)
    x = np.where(np.abs(x.astype(np.float64) * a[:, None]) <= 8192.0, x, np.float32(0.5))
    out = torch.zeros(Cn * L, device=gpu)
    qtts.Kernels.xgemm_func(out, _dev(x, gpu), 0, _dev(a, gpu), _dev(ib, gpu))
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(Cn, L).astype(np.float64)
    err = np.abs(got - X.snake64(x, a[:, None], ib[:, None]))
    bound = X.d_snake(x, a[:, None], ib[:, None])
    print(f"err / bound  snake1 (sin2)                    {np.max(err / bound):.4f}")
    assert np.all(err <= bound)
    for fn, lo, hi, f64, name in ((1, -16.0, 16.0, np.exp, "expf"), (2, -12.0, 12.0, np.tanh, "tanhf")):
        v = _grid(lo, hi, 1 << 20)
        out = torch.zeros(v.size, device=gpu)
        qtts.Kernels.xgemm_func(out, _dev(v, gpu), fn)
        torch.cuda.synchronize()
        got, ref = out.cpu().numpy().astype(np.float64), f64(v.astype(np.float64))
        m = float(np.max(np.abs(got - ref) / ref)) if fn == 1 else float(np.max(np.abs(got - ref)))
        print(f"measured  {name}: largest {'relative' if fn == 1 else 'absolute'} error {m:.3e}")
        assert m <= X.FUNC_ERR_MAX


def test_zz_every_kernel_and_both_reduces_ran(gpu):
    """from the reports of the cases above (runs last in this module): each of
    the six kernels ran, each with splits > 1 (the conv kernels through
    k_conv_reduce, k_xlin / k_xgemm through k_xg_reduce, k_xgemv's K slots)"""
    for path in range(6):       # (run on its own, or out of order: the first split case of the kernel)
        if _SEEN.get(path, 0) <= 1:
            check_case(gpu, next(sp for sp in CASES if sp.path == path and sp.splits > 1))
    for k in sorted(_RATIO):
        print(f"err / bound  {k:40s} {_RATIO[k]:.4f}")
    assert sorted(_SEEN) == list(range(6)), _SEEN
    assert all(v > 1 for v in _SEEN.values()), _SEEN
