"""The one-plane prefill GEMM (k_round1 + k_pgemmh<2> / <4>, k_pgemmh.hip)
through Kernels.rows_gemm_case with force 3 / 4, against the float64 reference
of rows_gemm_ref.py, in test_gpu_rows_gemm.py's buffers (NaN behind every x
row, sentinels behind y, the partials and the plane scratch).

Shapes: 17 rows (one row tile, 111 pad rows), 129 (a second tile holding one
row), 257; R 32 (less than a weight tile: the clamped row R - 1), 96 and 288
(no tile multiple); C 256 (four stages, no split), 512 (kz 2), 2048 (kz 8).

The bound.  The kernel multiplies bf16(a) by W exactly and sums in fp32, a = x
or x * inv * norm_w in fp32.  Nearest-even rounding to bf16 (8 significand
bits) moves a by at most half an ulp, ulp(a) <= 2^-7 |a|, and W is bf16
already, so |sum_k bf16(a_k) w_k - sum_k a_k w_k| <= 2^-8 sum_k |a_k| |w_k| =
b_round.  Every element must lie within b_acc + b_round of float64, b_acc the
exact kernels' own bound, pushed through the epilogue as theirs is.

b_round is ~2000 b_acc and cannot see a dropped stage, a wrong swizzle or a
wrong split column on a few elements.  The exact-sum cases can: integer x and
W (|x| <= 7, |w| <= 3: on the bf16 grid, every partial sum below 2^24), no
norm, so the result equals float64 bit for bit in any order.
Largest err / bound on one MI355X: <2> 0.149, <4> 0.039, split 0.050 / 0.136.
"""
import numpy as np
import pytest

import qtts
import rows_gemm_ref as G
from attn_ref import rne_bf16
from rows_gemm_ref import RESID, SWIGLU, Case
from test_gpu_rows_gemm import run_case

pytestmark = pytest.mark.gpu

H2, H4 = qtts.RG_NAMES_BF16
F_H128, F_H256, _RATIO = 3, 4, {}


def _case(M, R, C, force, kz=1, **kw):
    Mp = (M + G.BM - 1) // G.BM * G.BM
    return Case(M, R, C, force=force, kernel=H2 if force == F_H128 else H4, kz=kz, part=kz * M * R if kz > 1 else 0,
                planes=kw.pop("planes", Mp * C), **kw)


ROUNDED = [   # each epilogue with and without the norm
    _case(17, 32, 256, F_H128), _case(17, 32, 256, F_H256, epi=SWIGLU, norm=True),
    _case(129, 96, 256, F_H128, epi=RESID, norm=True), _case(257, 288, 256, F_H256, epi=SWIGLU),
    _case(129, 96, 512, F_H128, kz=2, epi=SWIGLU, norm=True), _case(257, 288, 512, F_H256, kz=2, norm=True),
    _case(17, 32, 2048, F_H128, kz=8, epi=RESID), _case(257, 96, 2048, F_H256, kz=8, epi=RESID, norm=True),
]
EXACT = [
    _case(129, 96, 256, F_H128, exact=True), _case(257, 288, 512, F_H256, kz=2, exact=True),
    _case(17, 32, 2048, F_H128, kz=8, exact=True), _case(257, 96, 2048, F_H256, kz=8, exact=True),
]
REFUSED = [
    ("C = 128", _case(129, 96, 128, F_H128)), ("R = 48", _case(129, 48, 256, F_H256)),
    ("16 rows", _case(16, 96, 256, F_H128)), ("a bias epilogue", _case(129, 96, 256, F_H128, epi=G.BIAS)),
    ("plane one element short", _case(129, 96, 256, F_H256, planes=256 * 256 - 1)),
]


def _ran(gpu, cs, d):
    c0 = qtts.Kernels.pgemmh_launches()
    ran, y, y0 = run_case(gpu, cs, d)
    assert ran and (ran["kernel"], ran["kz"], ran["block"]) == (cs.kernel, cs.kz, 256 if cs.kernel == H2 else 512), ran
    assert qtts.Kernels.pgemmh_launches() == c0 + 1
    return y, y0


@pytest.mark.parametrize("cs", ROUNDED, ids=[cs.id() for cs in ROUNDED])
def test_within_the_rounding_bound(gpu, cs):
    d, _, _ = G.reference(cs)
    xn, W = G.normed64(cs, d), G.w64(d)
    acc, absdot = xn @ W.T, np.abs(xn) @ np.abs(W).T
    b = G.C_DOT * absdot + G.C_ABS + (G.C_NORM * np.abs(acc) if cs.norm else 0.0) + 2.0 ** -8 * absdot
    ref, bound = G.epilogue(cs, d, acc, b)
    y, y0 = _ran(gpu, cs, d)
    ok, ratio, why = G.check(cs, y, y0, ref, bound)
    name = cs.kernel + (" split" if cs.kz > 1 else "")
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print(f"err / bound  {ratio:.4f}  {cs.id()}   largest so far: {_RATIO}")
    assert ok, (cs.id(), why, ratio)


@pytest.mark.parametrize("cs", EXACT, ids=[cs.id() for cs in EXACT])
def test_integer_inputs_equal_float64(gpu, cs):
    rng = np.random.default_rng(cs.M * 7 + cs.C)
    x, W = (rng.integers(-a, a + 1, (n, cs.C)).astype(np.float32) for a, n in ((7, cs.M), (3, cs.R)))
    d = {"x": x, "W": rne_bf16(W).reshape(cs.R, cs.C), "y0": np.zeros((cs.M, cs.R), np.float32)}
    ref = x.astype(np.float64) @ W.astype(np.float64).T
    assert np.array_equal(G.w64(d), W) and np.abs(x).astype(np.float64).sum(1).max() * 3 < 2.0 ** 24
    y, y0 = _ran(gpu, cs, d)
    ok, n, why = G.check(cs, y, y0, ref, None)
    assert ok, (cs.id(), why, n, np.argwhere(y[:cs.M, :cs.R].astype(np.float64) != ref)[:16].tolist())


@pytest.mark.parametrize("what,cs", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shapes_launch_nothing(gpu, what, cs):
    d = G.make_inputs(cs)
    c0 = qtts.Kernels.pgemmh_launches()
    ran, y, y0 = run_case(gpu, cs, d)
    assert ran is None and qtts.Kernels.pgemmh_launches() == c0, what
    assert np.array_equal(y.view(np.uint32), y0.view(np.uint32)), what
