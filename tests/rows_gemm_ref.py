"""The float64 reference, the error bound, the exact-plane inputs and the
buffer check every test of the multi-row GEMMs shares (k_mgemm.hip, k_pgemm.hip
through qtts_hip_rows_gemm_case: test_gpu_rows_gemm.py on the device,
test_rows_gemm_ref.py without one).

The operation, in float64 from the inputs as given (bf16 weights widened
exactly, fp32 activations or bf16 table rows gathered by id):

    xn[m][c] = x[m][c]                                             no norm
             = x[m][c] / sqrt(mean_c x[m][c]^2 + eps) * norm_w[c]  RMSNorm
    acc[m][r] = sum_c A[r][c] xn[m][c]
    y = acc | acc + bias | silu(acc + bias) | y0 + acc | silu(gate) * up

with gate / up the rows q*8 + j / q*8 + 4 + j of acc (output q*4 + j).

The bound is the project's own, no new constant (test_gpu_kernels.py's
gemv_bound, test_decode_matvec_batch's norm term, test_resident_matvec's
SwiGLU propagation, xgemm_ref.py's epilogue figure EPS_OP = 2e-7):

    b_acc = 2e-6 * sum_c |A[r][c] xn[m][c]| + 1e-6      (+ 1e-5 |acc| with a norm)
    store             b_acc
    +bias, y0 + acc   b_acc + 2e-7 |y|
    silu(acc + bias)  1.1 b_acc + 2e-7 |y|               (|silu'| <= 1.1)
    SwiGLU            (b_gate + b_up) (|up| + |gate| + 1) + 2e-7 |y|

What this bound cannot see, and the exact-plane inputs can: both kernels write
each fp32 activation as three bf16 planes x1 + x2 + x3 and claim an fp32
product up to summation order.  On standard-normal x and weights of scale
1/sqrt(K) a dropped THIRD plane moves the result by at most 0.21 of the bound
(a sequential fp32 sum reaches 0.095; a dropped second plane 100 times the
bound), so a kernel that loses, misroutes or double-counts the third plane in
one tile, stage parity or split column passes every bound test.  exact_inputs()
builds inputs whose planes are known and whose every partial sum is exact in
fp32, so the device result must equal the float64 one bit for bit whatever the
summation order or split:

    x = a + b + c,  a in +-1.5, b in +-1.5 * 2^-9, c in {-1, 0, 1} * 2^-18
    each weight row: at most 15 nonzeros, each +-1, placed by construction so
    that every column is hit by some row (15 R >= C)

Under f2bf_rn the planes are exactly a, b and c (other choices, a = +-1 or c at
2^-17, land on rounding ties); every product and partial sum is a multiple of
2^-18 below 32, i.e. at most 23 significand bits.  The builder asserts all of
this.
"""
import zlib
from dataclasses import dataclass, replace

import numpy as np

from attn_ref import rne_bf16, widen
from xgemm_ref import EPS_OP, planes

C_DOT, C_ABS, C_NORM = 2e-6, 1e-6, 1e-5
STORE, BIAS, BIAS_SILU, RESID, SWIGLU = range(5)
EPI_NAMES = ["store", "bias", "bias_silu", "resid", "swiglu"]
RG_NAMES = ["k_mgemm<1,1>", "k_mgemm<2,1>", "k_mgemm<4,1>", "k_mgemm<4,2>", "k_mgemm<4,4>", "k_pgemm<2>", "k_pgemm<4>"]
F_AUTO, F_MGEMM, F_PGEMM128, F_PGEMM256 = -1, 0, 1, 2

EPS = 1e-6
SENTINEL = np.float32(12345.678)   # prefill of every output element a kernel must not write
PAD_X = 4                          # NaN floats behind every x row (ldx = C + PAD_X)
PAD_Y = 3                          # sentinel floats behind every y row
ROWS_Y = 2                         # sentinel rows behind the last y row
TAIL = 64                          # sentinel elements behind the stated part / planes / inv sizes
TABLE_ROWS = 50
BM = 128                           # k_pgemm's row tile


@dataclass(frozen=True)
class Case:
    """One projection: M rows, weights [R][C].  src 'x' | 'tab' (bf16 table by
    ids at stride bstride).  force as qtts_hip_rows_gemm_case takes it.  part:
    the stated split workspace in floats.  planes: True = exactly the plane
    scratch k_pgemm needs, False = none, an int = that many elements.  kernel /
    kz: what must be reported.  exact: the exact-plane inputs."""
    M: int
    R: int
    C: int
    epi: int = STORE
    norm: bool = False
    src: str = "x"
    bstride: int = 1
    force: int = F_MGEMM
    kernel: str = ""
    kz: int = 1
    part: int = 0
    planes: object = False
    exact: bool = False
    seed: int = 0

    @property
    def nout(self):
        return self.R // 2 if self.epi == SWIGLU else self.R

    @property
    def plane_elems(self):
        if self.planes is True:
            return 3 * ((self.M + BM - 1) // BM * BM) * self.C
        return int(self.planes)

    def id(self):
        s = f"M{self.M}-R{self.R}-C{self.C}-{EPI_NAMES[self.epi]}" + ("-norm" if self.norm else "")
        s += (f"-tab{self.bstride}" if self.src == "tab" else "") + ("-exact" if self.exact else "")
        s += f"-f{self.force}-ws{self.part}" + (f"-pl{self.plane_elems}" if self.planes is not True and self.planes else "")
        return s + f"-{self.kernel}x{self.kz}" + (f"-s{self.seed}" if self.seed else "")


# ------------------------------------------------------------------ inputs
def exact_inputs(M, R, C, rng):
    """(W bits [R][C], x fp32 [M][C], (a, b, c)) of the exact-plane instrument;
    asserts the conditions the docstring states"""
    assert 15 * R >= C, "every column needs a nonzero of some weight row"
    a = 1.5 * rng.choice([-1.0, 1.0], (M, C))
    b = 1.5 * 2.0 ** -9 * rng.choice([-1.0, 1.0], (M, C))
    c = 2.0 ** -18 * rng.choice([-1.0, 0.0, 1.0], (M, C))
    x64 = a + b + c
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    for got, want in zip(planes(x), (a, b, c)):
        assert np.array_equal(got, want), "the planes do not come out as designed"
    # row r's j-th nonzero at column ((15 r + j) P) mod C, P odd and prime to
    # every C in use: a bijection of Z_C, so the first C of the 15 R indices
    # cover every column, and a row's 15 are distinct and spread over K
    P = 7919
    assert np.gcd(P, C) == 1
    W = np.zeros((R, C))
    idx = (np.arange(R)[:, None] * 15 + np.arange(15)[None, :])
    cols = (idx * P) % C
    sign = rng.choice([-1.0, 1.0], (R, 15))
    np.put_along_axis(W, cols, sign, axis=1)
    assert np.all((W != 0).sum(1) == min(15, C)) and np.all((W != 0).any(0)), "a column is hit by no weight row"
    assert np.max(np.abs(x64) @ np.abs(W).T) < 32.0
    ref = x64 @ W.T
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the reference is not fp32-exact"
    assert np.array_equal(np.round(ref * 2.0 ** 18), ref * 2.0 ** 18)
    Wb = rne_bf16(W.astype(np.float32)).reshape(R, C)
    assert np.array_equal(widen(Wb).astype(np.float64).reshape(R, C), W)
    return Wb, x, (a, b, c)


def make_inputs(cs):
    """inputs of a case, deterministic in it: W bits [R][C]; x fp32 [M][C], or
    table bits [TABLE_ROWS][C] and ids [M * bstride] (row m's id at m *
    bstride, other rows' ids between them); norm_w; bias; y0
    (the residual, or zeros)"""
    rng = np.random.default_rng(zlib.crc32(repr((cs.M, cs.R, cs.C, cs.epi, cs.norm, cs.src, cs.bstride, cs.exact,
                                                 cs.seed)).encode()))
    M, R, C = cs.M, cs.R, cs.C
    d = {}
    if cs.exact:
        assert cs.src == "x" and not cs.norm and cs.epi == STORE
        d["W"], d["x"], d["abc"] = exact_inputs(M, R, C, rng)
    else:
        d["W"] = rne_bf16((rng.standard_normal((R, C)) / np.sqrt(C)).astype(np.float32)).reshape(R, C)
        if cs.src == "x":
            d["x"] = (rng.standard_normal((M, C)) * (2.0 if cs.norm else 1.0)).astype(np.float32)
        else:
            d["table"] = rne_bf16(rng.standard_normal((TABLE_ROWS, C)).astype(np.float32)).reshape(TABLE_ROWS, C)
            d["ids"] = rng.integers(0, TABLE_ROWS, M * cs.bstride).astype(np.int32)
    if cs.norm:
        d["norm_w"] = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    if cs.epi in (BIAS, BIAS_SILU):
        d["bias"] = rng.standard_normal(R).astype(np.float32)
    d["y0"] = rng.standard_normal((M, cs.nout)).astype(np.float32) if cs.epi == RESID else np.zeros((M, cs.nout), np.float32)
    return d


def source(cs, d):
    """the fp32 activation rows [M][C] a case reads (table rows widened exactly)"""
    if cs.src == "x":
        return d["x"]
    return widen(d["table"][d["ids"][::cs.bstride]]).reshape(cs.M, cs.C)


def w64(d):
    return widen(d["W"]).astype(np.float64).reshape(d["W"].shape)


# ------------------------------------------------------------------ float64 reference and bound
def silu64(g):
    return g / (1.0 + np.exp(-g))


def normed64(cs, d):
    x = source(cs, d).astype(np.float64)
    if not cs.norm:
        return x
    return x / np.sqrt((x ** 2).mean(1, keepdims=True) + EPS) * d["norm_w"].astype(np.float64)


def epilogue(cs, d, acc, b_acc):
    """(y, bound) [M][nout] from the accumulated [M][R]"""
    if cs.epi == STORE:
        return acc, b_acc
    if cs.epi == BIAS:
        y = acc + d["bias"].astype(np.float64)
        return y, b_acc + EPS_OP * np.abs(y)
    if cs.epi == BIAS_SILU:
        y = silu64(acc + d["bias"].astype(np.float64))
        return y, 1.1 * b_acc + EPS_OP * np.abs(y)
    if cs.epi == RESID:
        y = d["y0"].astype(np.float64) + acc
        return y, b_acc + EPS_OP * np.abs(y)
    M = acc.shape[0]
    q, qb = acc.reshape(M, -1, 2, 4), b_acc.reshape(M, -1, 2, 4)
    g, u = q[:, :, 0, :].reshape(M, -1), q[:, :, 1, :].reshape(M, -1)
    y = silu64(g) * u
    bsum = qb[:, :, 0, :].reshape(M, -1) + qb[:, :, 1, :].reshape(M, -1)
    return y, bsum * (np.abs(u) + np.abs(g) + 1.0) + EPS_OP * np.abs(y)


_CACHE = {}


def reference(cs, keep=True):
    """(inputs, y, bound) of a case, computed once and shared (read-only);
    the exact-plane cases' bound is zero: their check is equality"""
    key = replace(cs, force=0, kernel="", kz=1, part=0, planes=False)
    if key in _CACHE:
        return _CACHE[key]
    d = make_inputs(cs)
    xn, W = normed64(cs, d), w64(d)
    acc = xn @ W.T
    b_acc = C_DOT * (np.abs(xn) @ np.abs(W).T) + C_ABS + (C_NORM * np.abs(acc) if cs.norm else 0.0)
    y, bound = epilogue(cs, d, acc, b_acc)
    if cs.exact:
        bound = np.zeros_like(y)
    for a in [v for v in d.values() if isinstance(v, np.ndarray)] + [y, bound]:
        a.setflags(write=False)
    if keep:
        _CACHE[key] = (d, y, bound)
    return d, y, bound


# ------------------------------------------------------------------ the output buffer and its check
def y_buffer(cs, d):
    """y as the device gets it: [M + ROWS_Y][nout + PAD_Y], the sentinel
    everywhere but the residual's rows"""
    y = np.full((cs.M + ROWS_Y, cs.nout + PAD_Y), SENTINEL, np.float32)
    if cs.epi == RESID:
        y[:cs.M, :cs.nout] = d["y0"]
    return y


def check(cs, y_after, y_before, ref, bound):
    """(ok, err / bound or the count of differing elements, what failed) of an
    output buffer: every element inside the bound (exact cases: equal to the
    float64 reference), everything outside [M][nout] bit-identical to before"""
    got = y_after[:cs.M, :cs.nout].astype(np.float64)
    mask = np.ones(y_after.shape, bool)
    mask[:cs.M, :cs.nout] = False
    if not np.array_equal(y_after.view(np.uint32)[mask], y_before.view(np.uint32)[mask]):
        return False, float("inf"), "wrote outside the output"
    if not np.all(np.isfinite(got)):
        return False, float("inf"), "not finite"
    if cs.exact:
        n = int(np.count_nonzero(got != ref))
        return n == 0, float(n), "differs from float64" if n else ""
    err = np.abs(got - ref)
    ratio = float(np.max(err / bound))
    ok = bool(np.all(err <= bound))
    return ok, ratio, "" if ok else "outside the bound"


# ------------------------------------------------------------------ the kernels' arithmetic in numpy
def split_columns(cs):
    """[(c0, c1)] the K range of each split column of the case (both kernels:
    kz contiguous ranges of C / kz)"""
    step = cs.C // cs.kz
    return [(z * step, (z + 1) * step) for z in range(cs.kz)]


def model(cs, d, mutate=None, fp32=False):
    """The y buffer the kernels' arithmetic gives: the activations normalised
    in fp32 as the kernels do, split into the three bf16 planes, the plane
    products summed in float64 (fp32 True: in fp32, split column by split
    column in order), the epilogue in float64 (fp32 True: rounded to fp32).
    mutate: one of the planted errors of test_rows_gemm_ref.py."""
    M, R, C = cs.M, cs.R, cs.C
    x = source(cs, d)
    if cs.norm:
        ss = (x.astype(np.float64) ** 2).sum(1)
        iv = (1.0 / np.sqrt(ss / C + EPS)).astype(np.float32)
        x = (x * iv[:, None]).astype(np.float32) * d["norm_w"][None, :]
    pl = planes(x.astype(np.float32))
    if mutate == "drop3":
        pl = pl[:2]
    if mutate == "drop2":
        pl = [pl[0], pl[2]]
    W = w64(d)
    kw = np.ones(C)
    if mutate == "last_stage":
        kw[C - 32:] = 0.0
    if mutate == "split_column":
        c0, c1 = split_columns(cs)[cs.kz - 1]
        kw[c0:c1] = 0.0
    Wk = W * kw[None, :]
    if fp32:
        acc = np.zeros((M, R), np.float32)
        for c0, c1 in split_columns(cs):
            part = np.zeros((M, R), np.float32)
            for p in pl:
                part += (p[:, c0:c1].astype(np.float32) @ Wk[:, c0:c1].T.astype(np.float32))
            acc = acc + part
        acc = acc.astype(np.float64)
    else:
        acc = sum(p @ Wk.T for p in pl)
    if mutate == "pad_row":
        # a pad row (k_split3 points it at row 0) not zeroed: its products land on the tile's last real row
        acc[M - 1] += sum(p[0] @ Wk.T for p in pl)
    if mutate == "gate_up":
        q = acc.reshape(M, -1, 2, 4).copy()
        q[:, 0] = q[:, 0, ::-1, :]
        acc = q.reshape(M, R)
    y, _ = epilogue(cs, d, acc, np.zeros_like(acc))
    out = y_buffer(cs, d)
    out[:M, :cs.nout] = y.astype(np.float32)
    if mutate == "clamped_row":
        out[:M, cs.nout] = out[:M, cs.nout - 1]   # the tile's row past R - 1, computed from the clamped weight row
    return out
