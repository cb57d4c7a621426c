"""The float64 reference, the error bound and the test inputs every test of the
codec's contraction kernels shares (test_gpu_xgemm.py, test_xgemm_ref.py, the
conv tests of test_gpu_kernels.py).

The reference computes one contraction from the fp32 inputs as given -- the
im2col of a causal conv, the per-phase gather of a transposed conv, or A W^T --
then the SnakeBeta prologue and the epilogue, all in float64.

The bound, per output element, in float64:

    b_acc = 2e-6 * sum_k |a_k| |b'_k| + 1e-6          (+ sum_k |a_k| d_snake(b_k) with a prologue)

2e-6 / 1e-6 are the GEMV tests' constants (test_gpu_kernels.py).  b' is the
float64 SnakeBeta of the input.  d_snake bounds the device's fp32 SnakeBeta
x' = x + ib * sin2(x * a) against the float64 one (derived, not measured):

    d_snake = |ib| * (5e-7 + 1.2e-7 * |x a|) + 1.2e-7 * |x'|

sin2's stated absolute error is 2.2e-7; the argument x * a is rounded once
(6e-8 |x a|) and passes through |d sin^2 / dr| <= 1; the product with ib and
the sum with x are two more roundings (6e-8 (|ib| + |x'|) at most); all with a
2x margin.  Inputs keep |x a| <= 8192, the range sin2 states.

The epilogue propagates b_acc by its Lipschitz factor L and adds 2e-7 of the
output for its own fp32 roundings (EPS_OP, about three roundings):

    bound = L * b_acc + 2e-7 |out|          (+ d_snake(acc + bias) for the snake epilogue)

    store, +bias[n], +bias[m], +bias +res            L = 1
    C += acc * vec[n], (acc + bias) vec[n] + res     L = |vec[n]|
    gelu_tanh(acc + bias)                            L = 1.13        (max |gelu_tanh'|)
    silu(aux) * acc                                  L = |silu(aux)|
    snake(acc + bias; a, ib)                         L = 1 + |ib a|

No measured constant enters the bound.  The device's expf (SiLU) and tanhf
(GELU) were measured against float64 with qtts_hip_xgemm_func over the range
of the tests' epilogue inputs (|expf argument| <= 16, |tanhf argument| <= 12,
2^20 points each) on an MI355X: expf largest relative error 8.2e-8, tanhf
largest absolute error 7.9e-8 -- inside the 2e-7, so nothing is added for them.
test_gpu_xgemm.py::test_device_functions repeats the measurement and fails
above FUNC_ERR_MAX = 1e-7 (half of EPS_OP; the other half is the epilogue's
remaining roundings), and holds snake with the GEMMs' own sin2 to d_snake.

The constants are not to be loosened to make a kernel pass:
test_xgemm_ref.py fails when the bound stops telling a dropped bf16-plane
product, a shifted tap, a wrong dilation / pad / tmin, a dropped channel stage
or split, swapped phases, a neighbour's SnakeBeta parameters, a transposed bias
index or a missing last row / column from the right answer.
"""
import zlib
from dataclasses import dataclass, replace

import numpy as np

from attn_ref import rne_bf16, widen

C_DOT, C_ABS = 2e-6, 1e-6
EPS_OP = 2e-7
FUNC_ERR_MAX = 1e-7               # device expf (relative) / tanhf (absolute): measured 8.2e-8 / 7.9e-8

XA_ROWS, XA_TRANS, XA_TCONV_W = 0, 1, 2
XB_WT, XB_CONV, XB_TCONV = 0, 1, 2
(XE_STORE, XE_BIAS_N, XE_BIAS_N_GELU, XE_SILU_MUL, XE_SCALE_RESID_N, XE_BIAS_T, XE_BIAS_GAMMA_RES_T, XE_BIAS_M,
 XE_BIAS_M_RES, XE_BIAS_M_SNAKE) = range(10)
XP_CONVB2, XP_CONVB4, XP_CONV, XP_XLIN, XP_XGEMV, XP_XGEMM = range(6)
T_MODES = (XE_BIAS_T, XE_BIAS_GAMMA_RES_T)

LM, RM = 80, 8                    # NaN margins (columns) left and right of a conv input row
SENTINEL = np.float32(12345.678)  # prefill of every output element a kernel must not write


@dataclass(frozen=True)
class Spec:
    """One contraction.  kind 'lin': C[M][N] = A[M][K] W[N][K]^T; 'conv': M = co,
    N = L, ci channels, Kw taps; 'tconv': kernel Kw, stride, N = L input frames
    (M x N*stride outputs).  hist: the input's left margin holds history
    (tmin = -halo).  part: split workspace elements.  force: kernel asked for
    (-1: the planner's choice).  path / splits: what must be reported."""
    kind: str
    M: int
    N: int
    K: int = 0
    ci: int = 0
    Kw: int = 1
    dil: int = 1
    stride: int = 1
    hist: bool = False
    snake: bool = False
    emode: int = XE_STORE
    amode: int = XA_ROWS
    bias: bool = True
    planted: bool = False
    part: int = 0
    force: int = -1
    path: int = -1
    splits: int = 1
    lda: int = 0                  # lin: 0 = K + 4 (rows) / M + 3 (trans)
    seed: int = 0

    @property
    def ntap(self):
        return self.Kw // self.stride if self.kind == "tconv" else self.Kw

    @property
    def halo(self):
        return (self.Kw - 1) * self.dil if self.kind == "conv" else self.ntap - 1

    @property
    def tmin(self):
        return -self.halo if self.hist else 0

    @property
    def kdim(self):
        return self.K if self.kind == "lin" else self.ci * self.ntap

    @property
    def ncol(self):
        """logical output columns"""
        return self.N * self.stride if self.kind == "tconv" else self.N

    def id(self):
        s = f"{self.kind}-M{self.M}-N{self.N}-"
        s += f"K{self.K}-a{self.amode}" if self.kind == "lin" else f"ci{self.ci}-k{self.Kw}-d{self.dil}-s{self.stride}"
        s += f"-e{self.emode}" + ("-hist" if self.hist else "") + ("-snake" if self.snake else "")
        s += ("" if self.bias else "-nobias") + ("-planted" if self.planted else "")
        s += (f"-ws{self.part}" if self.part else "") + f"-f{self.force}-p{self.path}x{self.splits}"
        return s + (f"-lda{self.lda}" if self.lda else "")


# ------------------------------------------------------------------ inputs
def _planted(rng, shape, sign, k_lo, k_hi):
    """+-(a + b + c): a = 2^k (k in [k_lo, k_hi]), b just under half a bf16 ulp of
    a (x 1 or 0.75), c = a (2^-18 + 2^-19): three nonzero bf16 planes, fp32-exact"""
    a = np.exp2(rng.integers(k_lo, k_hi + 1, shape).astype(np.float64))
    b = a * (2.0 ** -8 - 2.0 ** -12) * rng.choice([1.0, 0.75], shape)
    c = a * (2.0 ** -18 + 2.0 ** -19)
    v = (a + b + c) * sign
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    return v.astype(np.float32)


def make_inputs(sp):
    """fp32 inputs of a case, deterministic in the spec: dict with
    lin: A [M][K], W [N][K];  conv: w [co][ci][Kw];  tconv: w [ci][co][Kw];
    conv / tconv: x [ci][LM + N + RM] (column LM + t holds x(t); the margins
    hold values too: the history, and what only a mutant or an over-read sees),
    sa / sb [ci] with a prologue;  bias, vec, aux, res / c0, ea, eb as the
    epilogue needs."""
    rng = np.random.default_rng(zlib.crc32(repr((sp.kind, sp.M, sp.N, sp.K, sp.ci, sp.Kw, sp.dil, sp.stride, sp.emode,
                                                 sp.amode, sp.snake, sp.hist, sp.planted, sp.seed)).encode()))
    M, N, K = sp.M, sp.N, sp.kdim
    d = {}
    if sp.kind == "lin":
        if sp.planted:
            sg = rng.choice([-1.0, 1.0], K)
            sg[112:] = 0.0                                      # at most 112 nonzero terms per output
            d["A"] = _planted(rng, (M, K), sg[None, :], -1, 1)
            d["W"] = _planted(rng, (N, K), sg[None, :], -2, 1)
        else:
            d["A"] = rng.standard_normal((M, K)).astype(np.float32)
            d["W"] = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    else:
        ci = sp.ci
        wshape = (M, ci, sp.Kw) if sp.kind == "conv" else (ci, M, sp.Kw)
        cax = (None, slice(None), None) if sp.kind == "conv" else (slice(None), None, None)
        if sp.planted:
            assert ci * sp.ntap <= 112 and not sp.snake
            sg = rng.choice([-1.0, 1.0], ci)
            d["w"] = _planted(rng, wshape, sg[cax], -2, 1)
            d["x"] = _planted(rng, (ci, LM + N + RM), sg[:, None], -1, 1)
        else:
            d["w"] = (rng.standard_normal(wshape) / np.sqrt(ci * sp.ntap)).astype(np.float32)
            d["x"] = rng.standard_normal((ci, LM + N + RM)).astype(np.float32)
        if sp.snake:
            d["sa"] = rng.uniform(0.5, 4.0, ci).astype(np.float32)
            d["sb"] = rng.uniform(0.2, 2.0, ci).astype(np.float32) * rng.choice([-1.0, 1.0], ci).astype(np.float32)
    e = sp.emode
    nb = N if e in (XE_BIAS_N, XE_BIAS_N_GELU, XE_BIAS_T, XE_BIAS_GAMMA_RES_T) else M
    if sp.bias and e != XE_STORE and e != XE_SILU_MUL and e != XE_SCALE_RESID_N:
        d["bias"] = rng.standard_normal(nb).astype(np.float32)
    if e in (XE_SCALE_RESID_N, XE_BIAS_GAMMA_RES_T):
        d["vec"] = rng.uniform(-1.5, 1.5, N).astype(np.float32)
    if e == XE_SILU_MUL:
        d["aux"] = (3.0 * rng.standard_normal((M, N))).astype(np.float32)
    if e in (XE_SCALE_RESID_N, XE_BIAS_M_RES):
        d["c0"] = rng.standard_normal((M, sp.ncol)).astype(np.float32)      # C before the call (res == C)
    if e == XE_BIAS_GAMMA_RES_T:
        d["c0"] = rng.standard_normal((N, M)).astype(np.float32)
    if e == XE_BIAS_M_SNAKE:
        d["ea"] = rng.uniform(0.5, 4.0, M).astype(np.float32)
        d["eb"] = rng.uniform(0.2, 2.0, M).astype(np.float32) * rng.choice([-1.0, 1.0], M).astype(np.float32)
    return d


# ------------------------------------------------------------------ float64 pieces
def snake64(x, a, ib):
    x, a, ib = (np.asarray(v, np.float64) for v in (x, a, ib))
    return x + ib * np.sin(x * a) ** 2


def d_snake(x, a, ib):
    x, a, ib = (np.asarray(v, np.float64) for v in (x, a, ib))
    assert np.all(np.abs(x * a) <= 8192.0)
    return np.abs(ib) * (5e-7 + 1.2e-7 * np.abs(x * a)) + 1.2e-7 * np.abs(snake64(x, a, ib))


def gelu64(u):
    return 0.5 * u * (1.0 + np.tanh(0.7978845608028654 * (u + 0.044715 * u ** 3)))


def silu64(g):
    return g / (1.0 + np.exp(-g))


def tap_offsets(sp, tap_shift=None, ddil=0, dpad=0):
    """input column of tap j at output n: t = n + off[j].  The keyword arguments
    are the self-test's mutations."""
    off = []
    for j in range(sp.ntap):
        o = j * (sp.dil + ddil) - (sp.halo + dpad) if sp.kind == "conv" else -j
        if tap_shift is not None and tap_shift[0] == j:
            o += tap_shift[1]
        off.append(o)
    return off


def gather(sp, Wm, xrow, dtmin=0, **mut):
    """Wm [M][K] (k = ic * ntap + j) times the conv operand of xrow [ci][LM + N +
    RM]: sum_j Wm[:, j::ntap] x(:, n + off[j]), zero outside [tmin, N)"""
    N, nt = sp.N, sp.ntap
    tmin = sp.tmin + dtmin
    out = np.zeros((Wm.shape[0], N))
    for j, o in enumerate(tap_offsets(sp, **mut)):
        n0, n1 = max(0, tmin - o), min(N, N - o)
        if n1 > n0:
            out[:, n0:n1] += Wm[:, j::nt] @ xrow[:, LM + n0 + o:LM + n1 + o]
    return out


def im2col(sp, xrow):
    """the dense [K][N] conv operand (row ic * ntap + j), for the small planted cases"""
    out = np.zeros((sp.ci, sp.ntap, sp.N))
    n = np.arange(sp.N)
    for j, o in enumerate(tap_offsets(sp)):
        ok = (n + o >= sp.tmin) & (n + o < sp.N)
        out[:, j, ok] = xrow[:, LM + n[ok] + o]
    return out.reshape(sp.ci * sp.ntap, sp.N)


def wmat(sp, w, phase=0):
    """[M][K] operand: conv w [co][ci][Kw] as given; transposed conv w [ci][co][Kw]:
    column ic * ntap + j holds w[ic][m][phase + j * stride]"""
    w = np.asarray(w, np.float64)
    if sp.kind == "conv":
        return w.reshape(sp.M, sp.ci * sp.Kw)
    return np.transpose(w[:, :, phase::sp.stride], (1, 0, 2)).reshape(sp.M, sp.ci * sp.ntap)


def split_ranges(sp, nsplit=None):
    """K ranges [(k0, k1)] each split of the case sums, as the kernels deal them"""
    nz = sp.splits if nsplit is None else nsplit
    K = sp.kdim
    if sp.kind != "lin":                       # contiguous input channels
        cpz = sp.ci // nz
        return [(z * cpz * sp.ntap, (z + 1) * cpz * sp.ntap) for z in range(nz)]
    if sp.path == XP_XGEMV:                    # 32-column blocks dealt round-robin: not contiguous
        return None
    st = 128 if sp.path == XP_XLIN else 32
    nst = (K + st - 1) // st
    return [(min(K, nst * z // nz * st), min(K, nst * (z + 1) // nz * st)) for z in range(nz)]


def accumulate(sp, d, kw=None, **mut):
    """(acc, b_acc) [M][ncol] in float64.  kw: optional per-k weights [K] on
    the terms (the self-test's dropped / doubled stages and splits); mut: gather's
    mutations, snake_roll (the neighbouring channel's SnakeBeta parameters)."""
    roll = mut.pop("snake_roll", 0)
    K = sp.kdim
    kw = np.ones(K) if kw is None else np.asarray(kw, np.float64)
    if sp.kind == "lin":
        A, W = d["A"].astype(np.float64) * kw[None, :], d["W"].astype(np.float64)
        acc = A @ W.T
        return acc, C_DOT * (np.abs(A) @ np.abs(W).T) + C_ABS
    x = d["x"].astype(np.float64)
    dx = None
    if sp.snake:
        sa, sb = np.roll(d["sa"], roll)[:, None], np.roll(d["sb"], roll)[:, None]
        dx = d_snake(x, sa, sb)
        x = snake64(x, sa, sb)
    s = sp.stride
    acc, bnd = np.zeros((sp.M, sp.ncol)), np.zeros((sp.M, sp.ncol))
    for ph in range(s):
        Wm = wmat(sp, d["w"], ph) * kw[None, :]
        acc[:, ph::s] = gather(sp, Wm, x, **mut)
        bnd[:, ph::s] = C_DOT * gather(sp, np.abs(Wm), np.abs(x), **mut) + C_ABS
        if dx is not None:
            bnd[:, ph::s] += gather(sp, np.abs(Wm), dx, **mut)
    return acc, bnd


def epilogue(sp, d, acc, b_acc, bias_swap=False):
    """(out, bound) in the logical layout [M][ncol] (T modes too: the caller
    transposes).  bias_swap: the self-test's bias[m] <-> bias[n] mutation."""
    e = sp.emode
    M, NC = acc.shape
    by_n = e in (XE_BIAS_N, XE_BIAS_N_GELU, XE_BIAS_T, XE_BIAS_GAMMA_RES_T)
    if "bias" in d:
        b = d["bias"].astype(np.float64)
        col = (np.arange(NC) // sp.stride)
        if by_n != bias_swap:
            bias = b[col % len(b)][None, :] * np.ones((M, 1))
        else:
            bias = b[np.arange(M) % len(b)][:, None] * np.ones((1, NC))
    else:
        bias = np.zeros_like(acc)
    u = acc + bias
    if e in (XE_STORE, XE_BIAS_N, XE_BIAS_T, XE_BIAS_M):
        out, lip, extra = u, 1.0, 0.0
    elif e == XE_BIAS_M_RES:
        out, lip, extra = u + d["c0"].astype(np.float64), 1.0, 0.0
    elif e == XE_SCALE_RESID_N:
        v = d["vec"].astype(np.float64)[None, :]
        out, lip, extra = d["c0"].astype(np.float64) + acc * v, np.abs(v), 0.0
    elif e == XE_BIAS_GAMMA_RES_T:
        v = d["vec"].astype(np.float64)[None, :]
        out, lip, extra = u * v + d["c0"].astype(np.float64).T, np.abs(v), 0.0
    elif e == XE_BIAS_N_GELU:
        out, lip, extra = gelu64(u), 1.13, 0.0
    elif e == XE_SILU_MUL:
        sl = silu64(d["aux"].astype(np.float64))
        out, lip, extra = sl * acc, np.abs(sl), 0.0
    elif e == XE_BIAS_M_SNAKE:
        a, ib = d["ea"].astype(np.float64)[:, None], d["eb"].astype(np.float64)[:, None]
        out, lip, extra = snake64(u, a, ib), 1.0 + np.abs(ib * a), d_snake(u, a, ib)
    else:
        raise ValueError(e)
    return out, lip * b_acc + EPS_OP * np.abs(out) + extra


_CACHE = {}


def reference(sp, keep=True):
    """(inputs, out, bound) of a case, computed once (the arrays are shared: do
    not write to them); keep False: not kept (the large shipped shapes)"""
    key = replace(sp, part=0, force=-1, path=-1, splits=1, lda=0)
    if key in _CACHE:
        return _CACHE[key]
    d = make_inputs(sp)
    acc, b_acc = accumulate(sp, d)
    out, bound = epilogue(sp, d, acc, b_acc)
    for a in list(d.values()) + [out, bound]:
        a.setflags(write=False)
    if keep:
        _CACHE[key] = (d, out, bound)
    return d, out, bound


def conv_reference(x, w, b, k, dil=1, stride=0):
    """(out, bound) of a plain causal conv (stride 0; w [co][ci][k]) or
    transposed conv (w [ci][co][k], trimmed to L * stride outputs) with bias,
    no history: what qtts_hip_causal_conv1d / qtts_hip_transposed_conv1d compute"""
    ci, L = x.shape
    kind = "tconv" if stride else "conv"
    M = w.shape[1] if stride else w.shape[0]
    sp = Spec(kind, M, L, ci=ci, Kw=k, dil=dil, stride=stride or 1, emode=XE_BIAS_M)
    xr = np.zeros((ci, LM + L + RM), np.float32)
    xr[:, LM:LM + L] = x
    d = {"x": xr, "w": np.asarray(w, np.float32), "bias": np.asarray(b, np.float32)}
    acc, b_acc = accumulate(sp, d)
    return epilogue(sp, d, acc, b_acc)


# ------------------------------------------------------------------ the 3-plane split in numpy
def planes(v):
    """the kernels' exact split: v == p1 + p2 + p3, each plane bf16 (float64 arrays)"""
    v = np.asarray(v, np.float32)
    p1 = widen(rne_bf16(v)).reshape(v.shape)
    e = (v - p1).astype(np.float32)
    p2 = widen(rne_bf16(e)).reshape(v.shape)
    p3 = widen(rne_bf16((e - p2).astype(np.float32))).reshape(v.shape)
    return [p.astype(np.float64) for p in (p1, p2, p3)]


KEPT = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]   # the six products with i + j <= 4 (1-based)


def operands(sp, d, phase=0):
    """dense fp32 (A [M][K], B [K][N]) of a prologue-free case (one phase)"""
    if sp.kind == "lin":
        return d["A"], d["W"].T
    return wmat(sp, d["w"], phase).astype(np.float32), im2col(sp, d["x"]).astype(np.float32)
