"""The float64 references, the error bounds, the inputs and the buffer layout
every kernel-level test of the voice-clone encoder kernels shares (k_enc.hip;
test_gpu_enc_kernels.py on the device, test_enc_kernel_ref.py on a CPU box).

References.  Plain numpy float64 from each operation's definition, computed
from the fp32 inputs as given: the conv pads each utterance with np.pad
(constant / reflect / edge), takes the strided, dilated windows and multiplies
by the weight matrix; nothing of the kernel's index remapping is repeated.

Bounds, per output element, in float64, from the project's constants only
(xgemm_ref.py: C_DOT 2e-6, C_ABS 1e-6 from the GEMV tests, EPS_OP 2e-7 for
about three fp32 roundings, FUNC_ERR_MAX 1e-7 for a device function):

    b_acc = C_DOT * sum_k |w_k| |x'_k| + C_ABS + sum_k |w_k| d_in(x_k)

    d_in  = 2^-24 |x + x2|          the fp32 sum of the Res2Net prologue (one rounding)
          + FUNC_ERR_MAX  (x' < 0)  the ELU prologue's expm1f (ELU has Lipschitz factor 1)

    bound = |vec[m]| * L * b_acc + EPS_OP * |out|

    L: none / ReLU / tanh(ReLU) 1, exact GELU 1.13 (max |gelu'|), sigmoid 0.25;
    vec: LayerScale (1 without); EPS_OP |out| covers bias, activation and residual.

Small kernels (x: input, L: valid length, w_t: softmax weight):

    k_row_mean   C_DOT * sum|x| / L + C_ABS                          (= b_mean)
    k_egemv      as the conv: L * (C_DOT * sum|w||x| + C_ABS) + EPS_OP |out|
    k_se_apply   EPS_OP * (|h s| + |out|)
    k_asp_stats  mean: b_mean.  variance: d_v = C_DOT * v + b_mean^2 (the sum about
                 a mean off by e is v + e^2 exactly); std: min(sqrt(d_v), d_v /
                 sqrt(v)) + EPS_OP * std, from |sqrt(v') - sqrt(v)| <= sqrt(|v' - v|)
                 and = |v' - v| / (sqrt(v') + sqrt(v)): finite for a constant channel.
    k_asp_pool   weights: r_t = 2^-24 |a_t - max| + FUNC_ERR_MAX (the rounded
                 argument, expf), w_t off by at most w_t * (r_t + sum_s w_s r_s +
                 C_DOT + EPS_OP) = d_w; mean: sum |x_t| d_w + C_DOT sum w|x| +
                 C_ABS; variance: sum (x_t - mean)^2 d_w + C_DOT v + b_mean^2;
                 std as above.
    k_ln_rows    b_mean, d_v as k_asp_stats; inv = 1 / sqrt(v + eps) off by inv *
                 d_v / (v + eps); |w| * (inv * (b_mean + 2^-24 |x|) + |x - mean| *
                 d_inv) + EPS_OP * (|y| + |y - b|)
    k_mel        log domain: d_acc / max(acc, 1e-5) + EPS_OP |out| + C_ABS with
                 d_acc = (C_DOT + EPS_OP) * sum fb * mag (all terms positive;
                 EPS_OP: the magnitude's roundings)
    k_rope_bt    2 * EPS_OP * (|a cs| + |c sn|)
    k_rows_bt, k_rvq_enc: equality

Device functions.  expf and tanhf are held to FUNC_ERR_MAX by
test_gpu_xgemm.py::test_device_functions.  erff (GELU) and expm1f (ELU) were
measured on an MI355X against float64 (math.erf, np.expm1) with
qtts_hip_enc_func over the range of these tests' arguments, 2^20 points each:
see MEASURED below.  test_gpu_enc_kernels.py::test_device_functions repeats the
measurement and holds both to FUNC_ERR_MAX, so nothing is added to the bound
beyond the FUNC_ERR_MAX term of d_in.

Exact-plane inputs.  k_econv splits both operands into three bf16 planes and
keeps six of the nine plane products, so full three-plane inputs on both sides
do not equal float64 (the three dropped products are nonzero: 1.2e-7 at M 70,
K 200, N 67).  Three instruments instead, each with no prologue and the plain
store: (A) three-plane weights, one-plane x; (B) one-plane weights,
three-plane x; (C) two planes each.  Planes +-1.5, +-1.5 * 2^-9, {-1, 0, 1} *
2^-18; at most 7 nonzeros per weight row, every k hit by some row.  Together
all six kept products are nonzero somewhere and no dropped product ever is;
every product and partial sum is a multiple of 2^-20 below 16, so any
summation order is exact in fp32 and the device result must equal the float64
reference bit for bit.  exact_operands asserts all of this.

Buffers.  Every buffer is fully allocated; NaN left and right of every input
row, in channels / columns outside the slice a case reads and behind every
utterance's valid length; SENTINEL in every output element a kernel must not
write (columns >= lout[b], rows >= M, other channel slices, the gap between
utterances, the tail of the split-K workspace).  An over-read shows as a NaN in
the result, a stray write as a changed sentinel.

run_model restates k_econv's arithmetic in numpy on those same buffers (three
bf16 planes of both operands, the six products in the kernel's order, fp32
accumulation per 16-wide MFMA, the split-K ranges summed in split order) with
the kernel's own index arithmetic; test_enc_kernel_ref.py shows that the
bounds pass it and fail each of its mutants.
"""
import math
import zlib
from dataclasses import dataclass, replace

import numpy as np

from xgemm_ref import C_ABS, C_DOT, EPS_OP, FUNC_ERR_MAX, KEPT, SENTINEL, planes

MEASURED = {   # MI355X, 2^20 points each, largest absolute error against float64
    "erff": (-6.0, 6.0, 7.93e-8),      # |GELU's erff argument| <= 6
    "expm1f": (-12.0, 0.0, 3.97e-8),    # the ELU prologue's negative inputs
}
F32_EPS = 2.0 ** -24

PAD_ZERO, PAD_REFLECT, PAD_REPLICATE = range(3)
ACT_NONE, ACT_RELU, ACT_RELU_TANH, ACT_GELU, ACT_SIGMOID = range(5)
LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_RELU_TANH: 1.0, ACT_GELU: 1.13, ACT_SIGMOID: 0.25}
NP_PAD = {PAD_ZERO: "constant", PAD_REFLECT: "reflect", PAD_REPLICATE: "edge"}

LM, RM = 24, 8          # NaN margin (columns, or rows of a time-major buffer) left / right of an input row
OPAD, OGAP = 5, 7       # sentinel columns right of an output row; sentinel floats between utterances
PART_TAIL = 64          # sentinel floats behind the split-K workspace
ISENT = -7              # sentinel of the int outputs


@dataclass(frozen=True)
class Conv:
    """One k_econv launch.  lin / lout per utterance.  tm_in: time-major input
    rows x[t][c] with xpad NaN columns behind the ci channels (else
    channel-major [C][L]); cin (c0, Ctot): the ci input channels are the slice
    c0.. of a Ctot-channel buffer; mono: one input channel shared by all taps
    (xc = 0, the STFT); tm_out: y[n][m] (yc = 1, yt = M + ypad); cout as cin.
    res: residual in place (res == y).  exact: None or the instrument 'A' /
    'B' / 'C'.  rows / kz: what the plan must report."""
    name: str
    M: int
    ci: int
    kw: int = 1
    stride: int = 1
    dil: int = 1
    padl: int = 0
    pmode: int = PAD_ZERO
    lin: tuple = ()
    lout: tuple = ()
    act_in: int = 0
    x2: bool = False
    tm_in: bool = False
    xpad: int = 0
    cin: tuple = None
    mono: bool = False
    tm_out: bool = False
    ypad: int = 0
    cout: tuple = None
    bias: bool = False
    bias2: bool = False
    act_out: int = ACT_NONE
    vec: bool = False
    res: bool = False
    exact: str = None
    rows: int = 0
    kz: int = 1
    seed: int = 0

    @property
    def K(self):
        return self.ci * self.kw

    @property
    def nb(self):
        return len(self.lin)

    @property
    def nmax(self):
        return max(self.lout)

    def id(self):
        s = f"{self.name}-M{self.M}-{self.ci}x{self.kw}-s{self.stride}d{self.dil}p{self.pmode}.{self.padl}"
        s += "-L" + ".".join(map(str, self.lin)) + f"-rows{self.rows}-kz{self.kz}"
        s += f"-e{int(self.bias)}{int(self.bias2)}{self.act_out}{int(self.vec)}{int(self.res)}"
        return s + (f"-exact{self.exact}" if self.exact else "")


# ------------------------------------------------------------------ inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _exact_values(rng, shape, nplanes):
    v = 1.5 * rng.choice([-1.0, 1.0], shape)
    if nplanes >= 2:
        v = v + 1.5 * 2.0 ** -9 * rng.choice([-1.0, 1.0], shape)
    if nplanes >= 3:
        v = v + 2.0 ** -18 * rng.choice([-1.0, 0.0, 1.0], shape)
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    return v.astype(np.float32)


EXACT_PLANES = {"A": (3, 1), "B": (1, 3), "C": (2, 2), "full": (3, 3)}   # (weights, x)


def make_inputs(cv):
    """fp32 inputs of a case, deterministic in it: w [M][K]; x [nb][ci][Lmax]
    (mono: [nb][1][Lmax]); x2 as x; bias [M]; bias2 [nb][M]; vec [M]; res
    [nb][M][nmax]"""
    rng = _rng(cv.name, cv.M, cv.ci, cv.kw, cv.stride, cv.dil, cv.padl, cv.pmode, cv.lin, cv.act_in, cv.x2, cv.exact,
               cv.seed)
    M, K, nb, Lm = cv.M, cv.K, cv.nb, max(cv.lin)
    cx = 1 if cv.mono else cv.ci
    d = {}
    if cv.exact:
        assert not (cv.act_in or cv.x2 or cv.bias or cv.bias2 or cv.act_out or cv.vec or cv.res)
        assert 7 * M >= K, "every k needs a nonzero of some weight row"
        pw, px = EXACT_PLANES[cv.exact]
        w = np.zeros((M, K), np.float32)
        cols = (np.arange(M)[:, None] * 7 + np.arange(7)[None, :]) % K
        np.put_along_axis(w, cols, _exact_values(rng, (M, 7), pw), axis=1)
        assert np.all((w != 0).sum(1) <= 7) and np.all((w != 0).any(0)), "a k is hit by no weight row"
        d["w"] = w
        d["x"] = _exact_values(rng, (nb, cx, Lm), px)
    else:
        d["w"] = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
        d["x"] = (rng.standard_normal((nb, cx, Lm)) * (1.5 if cv.act_in else 1.0)).astype(np.float32)
    if cv.x2:
        d["x2"] = rng.standard_normal((nb, cx, Lm)).astype(np.float32)
    if cv.bias:
        d["bias"] = rng.standard_normal(M).astype(np.float32)
    if cv.bias2:
        d["bias2"] = rng.standard_normal((nb, M)).astype(np.float32)
    if cv.vec:
        d["vec"] = (rng.uniform(0.5, 1.5, M) * rng.choice([-1.0, 1.0], M)).astype(np.float32)
    if cv.res:
        d["res"] = rng.standard_normal((nb, M, cv.nmax)).astype(np.float32)
    return d


# ------------------------------------------------------------------ float64 reference and bound
def elu64(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))


def act64(act, u):
    if act == ACT_RELU:
        return np.maximum(u, 0.0)
    if act == ACT_RELU_TANH:
        return np.tanh(np.maximum(u, 0.0))
    if act == ACT_GELU:
        return 0.5 * u * (1.0 + np.vectorize(math.erf)(u * math.sqrt(0.5)))
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-u))
    return u


def windows(cv, xb, L, lout, fill_mode=None):
    """[K][lout] conv operand of one utterance from xb [cx][>= L] (float64):
    np.pad by the case's mode, then the strided, dilated windows"""
    x = xb[:, :L]
    need = (lout - 1) * cv.stride + (cv.kw - 1) * cv.dil + 1
    padr = max(0, need - cv.padl - L)
    mode = NP_PAD[cv.pmode] if fill_mode is None else fill_mode
    if mode == "reflect":
        assert cv.padl < L and padr < L
    xp = np.pad(x, ((0, 0), (cv.padl, padr)), mode=mode)
    idx = np.arange(lout)[None, :] * cv.stride + np.arange(cv.kw)[:, None] * cv.dil      # [kw][lout]
    win = xp[:, idx]                                                                     # [cx][kw][lout]
    if cv.mono:
        assert cv.ci == 1
    return win.reshape(cv.K, lout)


def conv_reference(cv, d):
    """(out, bound), lists over utterances of [M][lout[b]] float64"""
    w = d["w"].astype(np.float64)
    outs, bounds = [], []
    for b in range(cv.nb):
        L, lo = cv.lin[b], cv.lout[b]
        s = d["x"][b].astype(np.float64)
        d_in = np.zeros_like(s)
        if cv.x2:
            s = s + d["x2"][b].astype(np.float64)
            d_in = d_in + F32_EPS * np.abs(s)
        if cv.act_in:
            d_in = d_in + np.where(s < 0, FUNC_ERR_MAX, 0.0)
            s = elu64(s)
        cols = windows(cv, s, L, lo)
        acc = w @ cols
        b_acc = C_DOT * (np.abs(w) @ np.abs(cols)) + C_ABS
        if cv.x2 or cv.act_in:
            b_acc = b_acc + np.abs(w) @ windows(cv, d_in, L, lo)
        u = acc
        if cv.bias:
            u = u + d["bias"].astype(np.float64)[:, None]
        if cv.bias2:
            u = u + d["bias2"][b].astype(np.float64)[:, None]
        v = act64(cv.act_out, u)
        lip = LIP[cv.act_out] * np.ones((cv.M, 1))
        if cv.vec:
            v = v * d["vec"].astype(np.float64)[:, None]
            lip = lip * np.abs(d["vec"].astype(np.float64))[:, None]
        if cv.res:
            v = v + d["res"][b, :, :lo].astype(np.float64)
        outs.append(v)
        bounds.append(lip * b_acc + EPS_OP * np.abs(v))
    return outs, bounds


def exact_operands(cv, d):
    """asserts the exact-plane conditions of the module docstring on the dense
    operands of every utterance; returns the float64 reference"""
    pw, px = EXACT_PLANES[cv.exact]
    w = d["w"]
    pa = planes(w)
    assert np.array_equal(pa[0] + pa[1] + pa[2], w.astype(np.float64))
    nz = w != 0
    assert np.all(np.abs(pa[0][nz]) == 1.5) and np.all(pa[0][~nz] == 0)
    assert np.all(np.abs(pa[1][nz]) == (1.5 * 2.0 ** -9 if pw >= 2 else 0.0))
    assert np.all(np.isin(pa[2] * 2.0 ** 18, [-1.0, 0.0, 1.0])) and (pw >= 3 or not pa[2].any())
    outs = []
    for b in range(cv.nb):
        cols = windows(cv, d["x"][b].astype(np.float64), cv.lin[b], cv.lout[b]).astype(np.float32)
        pb = planes(cols)
        assert np.array_equal(pb[0] + pb[1] + pb[2], cols.astype(np.float64))
        assert np.all(np.isin(np.abs(pb[0]), [0.0, 1.5]))
        assert np.all(np.isin(np.abs(pb[1]), [0.0, 1.5 * 2.0 ** -9])) and (px >= 2 or not pb[1].any())
        assert np.all(np.isin(pb[2] * 2.0 ** 18, [-1.0, 0.0, 1.0])) and (px >= 3 or not pb[2].any())
        # no dropped product is nonzero; the kept six sum to the float64 product
        for i in range(3):
            for j in range(3):
                if (i, j) not in KEPT:
                    assert not (np.abs(pa[i]) @ np.abs(pb[j])).any(), "a dropped plane product is nonzero"
        six = sum(pa[i] @ pb[j] for i, j in KEPT)
        ref = w.astype(np.float64) @ cols.astype(np.float64)
        assert np.array_equal(six, ref)
        # every product is a multiple of 2^-20, the absolute sum stays below 16:
        # every partial sum in any order is fp32-exact
        for i, j in KEPT:
            pr = np.unique(pa[i])[:, None] * np.unique(pb[j])[None, :]
            assert np.array_equal(np.round(pr * 2.0 ** 20), pr * 2.0 ** 20)
        assert np.max(np.abs(w.astype(np.float64)) @ np.abs(cols.astype(np.float64))) < 16.0
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the reference is not fp32-exact"
        outs.append(ref)
    return outs


_CACHE = {}


def reference(cv):
    """(inputs, outs, bounds) of a case, computed once and shared: read only"""
    key = replace(cv, rows=0, kz=1, xpad=0, ypad=0, cin=None, cout=None, tm_in=False, tm_out=False)
    if key not in _CACHE:
        d = make_inputs(cv)
        outs, bounds = conv_reference(cv, d)
        if cv.exact:
            ex = exact_operands(cv, d)
            for a, e in zip(outs, ex):
                assert np.array_equal(a, e)
        for a in list(d.values()) + outs + bounds:
            a.setflags(write=False)
        _CACHE[key] = (d, outs, bounds)
    return _CACHE[key]


# ------------------------------------------------------------------ buffers
def layout(cv, d):
    """The case's flat fp32 buffers and its descriptor fields.  Returns a dict:
    buffers 'w', 'x', 'x2', 'y', 'bias', 'bias2', 'vec' (numpy, flat); 'x_off' /
    'y_off' (floats from the buffer start to the element (b 0, c 0, t 0));
    xb, xc, xt, yb, yc, yt, rb, rc, rt, bias2_b."""
    nb, Lm, nmax, M = cv.nb, max(cv.lin), cv.nmax, cv.M
    nan = np.float32(np.nan)
    lo = {}
    cx = 1 if cv.mono else cv.ci
    c0, Ct = cv.cin if cv.cin else (0, cx)

    def xbuf(src):
        if cv.tm_in:
            xt = Ct + cv.xpad
            buf = np.full((nb, LM + Lm + RM, xt), nan, np.float32)
            for b in range(nb):
                buf[b, LM:LM + cv.lin[b], c0:c0 + cx] = src[b][:, :cv.lin[b]].T
            lo.update(xb=(LM + Lm + RM) * xt, xc=1, xt=xt, x_off=LM * xt + c0)
        else:
            row = LM + Lm + RM
            buf = np.full((nb, Ct, row), nan, np.float32)
            for b in range(nb):
                buf[b, c0:c0 + cx, LM:LM + cv.lin[b]] = src[b][:, :cv.lin[b]]
            lo.update(xb=Ct * row, xc=0 if cv.mono else row, xt=1, x_off=c0 * row + LM)
        return buf.reshape(-1)

    lo["x"] = xbuf(d["x"])
    if cv.x2:
        lo["x2"] = xbuf(d["x2"])
    m0, Mt = cv.cout if cv.cout else (0, M)
    if cv.tm_out:
        yt = Mt + cv.ypad
        yb = (nmax + 2) * yt + OGAP
        lo.update(yb=yb, yc=1, yt=yt, y_off=m0)
    else:
        row = nmax + OPAD
        yb = (Mt + 1) * row + OGAP
        lo.update(yb=yb, yc=row, yt=1, y_off=m0 * row)
    y = np.full(nb * yb + 8, SENTINEL, np.float32)
    lo["y"] = y
    lo["valid"] = valid = np.zeros(y.shape, bool)
    lo["yidx"] = []
    for b in range(nb):
        n = np.arange(cv.lout[b])
        idx = lo["y_off"] + b * lo["yb"] + np.arange(M)[:, None] * lo["yc"] + n[None, :] * lo["yt"]
        assert not valid[idx].any()
        valid[idx] = True
        lo["yidx"].append(idx)
        if cv.res:
            y[idx] = d["res"][b][:, :cv.lout[b]]
    lo.update(rb=lo["yb"], rc=lo["yc"], rt=lo["yt"])
    lo["w"] = d["w"].reshape(-1)
    for k in ("bias", "vec"):
        if k in d:
            lo[k] = np.concatenate([d[k], np.full(4, nan, np.float32)])
    if cv.bias2:
        lo["bias2_b"] = M + 3
        b2 = np.full((nb, M + 3), nan, np.float32)
        b2[:, :M] = d["bias2"]
        lo["bias2"] = b2.reshape(-1)
    return lo


def check(cv, lo, y_after, ref=None):
    """every valid output within the bound (exact cases: bit-equal to the
    float64 reference), everything else untouched bit for bit.  Returns the
    largest err / bound."""
    d, outs, bounds = reference(cv) if ref is None else ref
    worst = 0.0
    for b in range(cv.nb):
        got = y_after[lo["yidx"][b]].astype(np.float64)
        assert np.all(np.isfinite(got)), (cv.id(), b, "NaN / inf in the output: an over-read or a missing write")
        if cv.exact:
            assert np.array_equal(got, outs[b]), (cv.id(), b, float(np.max(np.abs(got - outs[b]))))
            continue
        err = np.abs(got - outs[b])
        ratio = float(np.max(err / bounds[b])) if err.size else 0.0
        assert np.all(err <= bounds[b]), (cv.id(), b, ratio, np.argwhere(~(err <= bounds[b]))[:4])
        worst = max(worst, ratio)
    y0 = lo["y"]
    keep = ~lo["valid"]
    assert np.array_equal(y_after.view(np.uint32)[keep], y0.view(np.uint32)[keep]), (cv.id(), "a stray write")
    return worst


# ------------------------------------------------------------------ k_econv restated in numpy
def f32(a):
    return np.asarray(a, np.float32)


def plan_model(cv, lo):
    """launch_econv's rule, restated: (rows, kz)"""
    nk = (cv.K + 31) // 32
    rows = (cv.kw == 1 and lo["xc"] == 1 and cv.stride == 1 and cv.padl == 0 and not cv.x2 and not cv.act_in
            and cv.K % 8 == 0 and lo["xt"] % 4 == 0 and lo["x_off"] % 4 == 0)
    tiles1 = (cv.nmax + 63) // 64 * ((cv.M + 63) // 64)
    kz = 1
    if rows:
        kz = min(4, nk // 4) if nk >= 8 else 1
    elif tiles1 < 256 and nk >= 8:
        kz = max(1, min(nk // 4, 16, (512 + tiles1 - 1) // tiles1))
    return int(rows), kz


def model_cols(cv, lo, b, mut=()):
    """fp32 [K][lout[b]] staged operand of utterance b, gathered from the flat
    buffers with the kernel's own index arithmetic (mut: the self-test's mutations)"""
    L, lout = cv.lin[b], cv.lout[b]
    stride = cv.stride + (1 if "stride" in mut else 0)
    dil = cv.dil + (1 if "dil" in mut else 0)
    k = np.arange(cv.K)
    ci, tap = k // cv.kw, k % cv.kw
    if "tap" in mut and cv.kw > 1:
        tap = np.where(tap == cv.kw - 1, tap + 1, tap)
    t = (np.arange(lout)[None, :] * stride - cv.padl) + (tap * dil)[:, None]
    ok = np.ones(t.shape, bool)
    out = (t < 0) | (t >= L)
    pmode = cv.pmode
    if pmode == PAD_REPLICATE and "replicate" in mut:
        pmode = PAD_ZERO
    if pmode == PAD_REFLECT:
        hi = 2 * L - 1 - t if "reflect" in mut else 2 * (L - 1) - t
        lo_ = -t - 1 if "reflect" in mut else -t
        t = np.where(t < 0, lo_, np.where(t >= L, hi, t))
    elif pmode == PAD_REPLICATE:
        t = np.clip(t, 0, L - 1)
    else:
        ok = ~out
    t = np.clip(t, -LM, L + RM - 1)          # a mutant's stray index stays inside the margins
    o = lo["x_off"] + b * lo["xb"] + (ci * lo["xc"])[:, None] + t * lo["xt"]
    v = lo["x"][o]
    if cv.x2 and "x2" not in mut:
        if cv.act_in and "elu_order" in mut:
            v = np.where(v > 0, v, np.expm1(v)).astype(np.float32) + lo["x2"][o]
        else:
            v = v + lo["x2"][o]
    if cv.act_in and not (cv.x2 and "elu_order" in mut):
        v = np.where(v > 0, v, np.expm1(np.minimum(v, 0)).astype(np.float32))
    return np.where(ok, f32(v), np.float32(0))


def model_mma(w, cols, kz, drop=None, last_step=True):
    """fp32 [M][N]: three planes of each operand, the six products in the
    kernel's order per 16-wide MFMA, fp32 accumulation, kz contiguous ranges of
    32-wide K-steps summed in split order.  drop: a (i, j) plane product left out."""
    M, K = w.shape
    Kp = (K + 31) // 32 * 32
    wp = np.zeros((M, Kp), np.float32)
    wp[:, :K] = w
    cp = np.zeros((Kp, cols.shape[1]), np.float32)
    cp[:K] = cols
    pa, pb = planes(wp), planes(cp)
    order = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]
    nk = Kp // 32
    total = np.zeros((M, cols.shape[1]), np.float32)
    for z in range(kz):
        acc = np.zeros_like(total)
        s0, s1 = nk * z // kz, nk * (z + 1) // kz
        if not last_step and z == kz - 1 and kz > 1 and nk % kz:
            s1 -= 1
        for s in range(s0, s1):
            for kg in range(2):
                sl = slice(s * 32 + kg * 16, s * 32 + kg * 16 + 16)
                for i, j in order:
                    if (i, j) != drop:
                        acc = f32(acc + f32(pa[i][:, sl] @ pb[j][sl]))
        total = f32(total + acc) if kz > 1 else acc
    return total


def model_act(act, v):
    v = f32(v)
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ACT_RELU_TANH:
        return f32(np.tanh(np.maximum(v, np.float32(0)).astype(np.float64)))
    if act == ACT_GELU:
        e = f32(np.vectorize(math.erf)(f32(v * np.float32(0.70710678118654752)).astype(np.float64)))
        return f32(f32(np.float32(0.5) * v) * f32(np.float32(1) + e))
    if act == ACT_SIGMOID:
        return f32(np.float32(1) / f32(np.float32(1) + f32(np.exp(-v.astype(np.float64)))))
    return v


def run_model(cv, lo, kz=None, mut=(), drop=None):
    """the launch on the case's buffers; returns y after"""
    y = lo["y"].copy()
    kz = plan_model(cv, lo)[1] if kz is None else kz
    w = lo["w"].reshape(cv.M, cv.K)
    for b in range(cv.nb):
        if cv.lout[b] == 0:
            continue
        acc = model_mma(w, model_cols(cv, lo, b, mut), kz, drop, last_step="last_step" not in mut)
        v = acc
        if cv.bias:
            v = f32(v + lo["bias"][:cv.M, None])
        if cv.bias2:
            bb = 0 if "bias2" in mut else b
            v = f32(v + lo["bias2"][bb * lo["bias2_b"]:bb * lo["bias2_b"] + cv.M, None])
        if cv.vec and "vec_order" in mut:
            v = model_act(cv.act_out, f32(v * lo["vec"][:cv.M, None]))
        else:
            v = model_act(cv.act_out, v)
            if cv.vec:
                v = f32(v * lo["vec"][:cv.M, None])
        idx = lo["yidx"][b]
        if cv.res:
            ridx = idx
            if "res_t" in mut:
                m, n = np.arange(cv.M)[:, None], np.arange(cv.lout[b])[None, :]
                ridx = (lo["y_off"] + b * lo["rb"] + n * lo["rc"] + m * lo["rt"]) % y.size
            v = f32(v + lo["y"][ridx])
        if "last_row" in mut:
            idx, v = idx[:-1], v[:-1]
        if "last_col" in mut:
            idx, v = idx[:, :-1], v[:, :-1]
        y[idx] = v
    return y


# ------------------------------------------------------------------ small kernels: references and bounds
def mean_ref(x):
    """(mean, bound) over the last axis"""
    x = np.asarray(x, np.float64)
    return x.mean(-1), C_DOT * np.abs(x).sum(-1) / x.shape[-1] + C_ABS


def std_bound(v, d_v, std):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(v > 0, d_v / np.sqrt(np.maximum(v, 1e-300)), np.inf)
    return np.minimum(np.sqrt(d_v), rel) + EPS_OP * std


def asp_stats_ref(x):
    """x [C][L] -> (mean, std, b_mean, b_std)"""
    x = np.asarray(x, np.float64)
    mean, b_mean = mean_ref(x)
    v = ((x - mean[:, None]) ** 2).mean(-1)
    std = np.sqrt(np.maximum(v, 1e-12))
    return mean, std, b_mean, std_bound(v, C_DOT * v + b_mean ** 2, std)


def asp_pool_ref(x, a):
    """x, logits a [C][L] -> (mean, std, b_mean, b_std)"""
    x, a = np.asarray(x, np.float64), np.asarray(a, np.float64)
    mx = a.max(-1, keepdims=True)
    e = np.exp(a - mx)
    w = e / e.sum(-1, keepdims=True)
    r = F32_EPS * np.abs(a - mx) + FUNC_ERR_MAX
    d_w = w * (r + (w * r).sum(-1, keepdims=True) + C_DOT + EPS_OP)
    mean = (w * x).sum(-1)
    b_mean = (np.abs(x) * d_w).sum(-1) + C_DOT * (w * np.abs(x)).sum(-1) + C_ABS
    dd = (x - mean[:, None]) ** 2
    v = (w * dd).sum(-1)
    std = np.sqrt(np.maximum(v, 1e-12))
    return mean, std, b_mean, std_bound(v, (dd * d_w).sum(-1) + C_DOT * v + b_mean ** 2, std)


def egemv_ref(W, x, bias, act):
    """W [R][C], x [nb][C] -> (out, bound) [nb][R]"""
    W, x = np.asarray(W, np.float64), np.asarray(x, np.float64)
    u = x @ W.T + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :])
    out = act64(act, u)
    return out, LIP[act] * (C_DOT * (np.abs(x) @ np.abs(W).T) + C_ABS) + EPS_OP * np.abs(out)


def se_apply_ref(h, s, res):
    h, s, res = (np.asarray(v, np.float64) for v in (h, s, res))
    hs = h * s[:, None]
    return hs + res, EPS_OP * (np.abs(hs) + np.abs(hs + res))


def ln_rows_ref(x, w, b, eps):
    x, w, b = (np.asarray(v, np.float64) for v in (x, w, b))
    mean, b_mean = mean_ref(x)
    xc = x - mean[:, None]
    v = (xc ** 2).mean(-1)
    inv = 1.0 / np.sqrt(v + eps)
    d_inv = inv * (C_DOT * v + b_mean ** 2) / (v + eps)
    y = xc * inv[:, None] * w + b
    bound = np.abs(w) * (inv[:, None] * (b_mean[:, None] + F32_EPS * np.abs(x)) + np.abs(xc) * d_inv[:, None])
    return y, bound + EPS_OP * (np.abs(y) + np.abs(y - b))


def mel_ref(spec, fb, flo, fhi):
    """spec [2 nf][T], fb [nm][nf] -> (mel, bound) [nm][T]; only the bins in
    [flo, fhi) of each filter count, as the filterbank is stored"""
    spec, fb = np.asarray(spec, np.float64), np.asarray(fb, np.float64)
    nf = fb.shape[1]
    mag = np.sqrt(spec[:nf] ** 2 + spec[nf:] ** 2 + np.float64(np.float32(1e-9)))
    f = np.arange(nf)[None, :]
    fbm = np.where((f >= np.asarray(flo)[:, None]) & (f < np.asarray(fhi)[:, None]), fb, 0.0)
    acc = fbm @ mag
    floor = np.float64(np.float32(1e-5))
    out = np.log(np.maximum(acc, floor))
    d_acc = (C_DOT + EPS_OP) * (np.abs(fbm) @ mag)
    return out, d_acc / np.maximum(acc, floor) + EPS_OP * np.abs(out) + C_ABS, acc


def rope_ref(x, nh, hd, T, cs, sn):
    """x [R][nh * hd] -> (out, bound), position = row % T"""
    x = np.asarray(x, np.float64)
    R, half = x.shape[0], hd // 2
    p = np.arange(R) % T
    q = x.reshape(R, nh, hd)
    a, c = q[:, :, :half], q[:, :, half:]
    c1, s1 = np.asarray(cs, np.float64)[p][:, None, :half], np.asarray(sn, np.float64)[p][:, None, :half]
    c2, s2 = np.asarray(cs, np.float64)[p][:, None, half:], np.asarray(sn, np.float64)[p][:, None, half:]
    out = np.concatenate([a * c1 - c * s1, c * c2 + a * s2], -1).reshape(R, nh * hd)
    bound = 2 * EPS_OP * np.concatenate([np.abs(a * c1) + np.abs(c * s1), np.abs(c * c2) + np.abs(a * s2)], -1)
    return out, bound.reshape(R, nh * hd)


# ------------------------------------------------------------------ k_rvq_enc
def rvq_ref(lat, psem, pac, cbk, nsem, nvalid, last_on_ties=False):
    """lat [nb][hid][T12], psem / pac [vq][hid], cbk [q][CB][vq] (float64 math)
    -> codes [nb * T12][nvalid], best [.][.] (smallest squared distance),
    margin [.][.] (second smallest - smallest), and whether every value of the
    chain stayed on the 1/8 grid within +-4 (the exact-grid condition)"""
    nb, hid, T12 = lat.shape
    z = np.transpose(np.asarray(lat, np.float64), (0, 2, 1)).reshape(nb * T12, hid)
    rows = z.shape[0]
    codes = np.zeros((rows, nvalid), np.int64)
    best, margin = np.zeros((rows, nvalid)), np.zeros((rows, nvalid))
    grid = True

    def on_grid(a, step, lim):
        return bool(np.all(np.round(a / step) * step == a) and np.all(np.abs(a) <= lim))
    for P, q0, q1 in ((psem, 0, nsem), (pac, nsem, nvalid)):
        r = z @ np.asarray(P, np.float64).T
        grid &= on_grid(r, 0.125, 4.0)
        for q in range(q0, q1):
            E = np.asarray(cbk[q], np.float64)
            dist = ((r[:, None, :] - E[None, :, :]) ** 2).sum(-1)
            idx = dist.shape[1] - 1 - np.argmin(dist[:, ::-1], 1) if last_on_ties else np.argmin(dist, 1)
            srt = np.sort(dist, 1)
            codes[:, q], best[:, q], margin[:, q] = idx, srt[:, 0], srt[:, 1] - srt[:, 0]
            r = r - E[idx]
            grid &= on_grid(r, 0.125, 4.0) and on_grid(E, 0.125, 4.0)
    return codes, best, margin, grid


def rvq_exact_inputs(nb, T12, CB, seed, hid=64, vq=32, nsem=1, nvalid=16):
    """The exact-grid case: latent multiples of 1/8 within +-2, projections with
    two +-1 per output, codebook entries multiples of 1/8 within +-4, so the
    projection, every squared distance (multiples of 1/64 below 2^11) and every
    residual (within +-4 all along the chain) are exact in fp32 in any order.  Exact duplicates of a row's winning
    entry are planted at index pairs (i, i + 1) across a wave boundary, (i, i +
    64), (i, i + 1024) and (1000, 1029): the lower index in a higher lane of a
    later wave.  Returns lat, psem, pac, cbk and the planted (row, q, i, j)."""
    rng = _rng("rvq-exact", nb, T12, CB, seed)
    lat = (rng.integers(-16, 17, (nb, hid, T12)) / 8.0).astype(np.float32)
    proj = []
    for _ in range(2):
        P = np.zeros((vq, hid), np.float32)
        for o in range(vq):
            P[o, rng.choice(hid, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
        proj.append(P)
    # one nonzero dim per entry and a zero entry per codebook: the winner never
    # lengthens a coordinate of the residual, so the chain stays within +-4
    cbk = np.zeros((nvalid, CB, vq), np.float32)
    for q in range(nvalid):
        cbk[q, np.arange(CB), rng.integers(0, vq, CB)] = rng.integers(-32, 33, CB) / 8.0
        cbk[q, rng.integers(0, CB)] = 0.0
    pairs = [(63, 64), (5, 69), (7, 1031), (1000, 1029)] if CB >= 2048 else [(63, 64), (5, 69)]
    rows = nb * T12
    z = np.transpose(lat.astype(np.float64), (0, 2, 1)).reshape(rows, hid)
    planted = []
    for P, qs in ((proj[0], range(0, nsem)), (proj[1], range(nsem, nvalid))):
        r = z @ P.astype(np.float64).T
        for q in qs:
            row = q % rows
            if q % 3 == 0:
                i, j = pairs[(q // 3) % len(pairs)]
                e = np.clip(r[row], -4.0, 4.0).copy()
                e[q % vq] += 0.125 if e[q % vq] < 4.0 else -0.125      # a winner at distance > 0
                cbk[q, i] = cbk[q, j] = e
                # nothing else as close: such entries move to a far corner
                near = ((r[row][None, :] - cbk[q].astype(np.float64)) ** 2).sum(-1) <= 1.0 / 64
                near[[i, j]] = False
                k = (q + 5) % vq
                far = np.zeros(vq, np.float32)
                far[k] = -4.0 if r[row][k] > 0 else 4.0
                cbk[q, near] = far
                planted.append((row, q, i, j))
            E = cbk[q].astype(np.float64)
            dist = ((r[:, None, :] - E[None, :, :]) ** 2).sum(-1)
            r = r - E[np.argmin(dist, 1)]
    codes, best, margin, grid = rvq_ref(lat, proj[0], proj[1], cbk, nsem, nvalid)
    assert grid, "the chain leaves the exact grid"
    for row, q, i, j in planted:
        assert codes[row, q] == i and margin[row, q] == 0.0, (row, q, i, j, codes[row, q])
    return lat, proj[0], proj[1], cbk, planted


def rvq_random_inputs(nb, T12, CB, seed, hid=64, vq=32, nvalid=16):
    rng = _rng("rvq-random", nb, T12, CB, seed)
    lat = rng.standard_normal((nb, hid, T12)).astype(np.float32)
    psem = (rng.standard_normal((vq, hid)) / np.sqrt(hid)).astype(np.float32)
    pac = (rng.standard_normal((vq, hid)) / np.sqrt(hid)).astype(np.float32)
    cbk = rng.standard_normal((nvalid, CB, vq)).astype(np.float32)
    for q in range(1, nvalid):
        cbk[q] *= np.float32(0.85 ** q)
    return lat, psem, pac, cbk


def check_codes(codes, ref, margins, best):
    """test_gpu_enc._check_codes' rule: a frame's first differing codebook may be
    a near tie within 1e-3 * (1 + best); at most max(1, frames // 10) such frames"""
    tol = 1e-3 * (1.0 + best)
    excused, bad = 0, []
    for f in range(codes.shape[0]):
        dq = np.nonzero(codes[f] != ref[f])[0]
        if dq.size == 0:
            continue
        q = int(dq[0])
        if margins[f, q] <= tol[f, q]:
            excused += 1
        else:
            bad.append((f, q, float(margins[f, q])))
    assert not bad, bad
    assert excused <= max(1, codes.shape[0] // 10), excused
    return excused


def rvq_model(lat, psem, pac, cbk, nsem, nvalid, last_on_ties=False):
    """k_rvq_enc restated in fp32 numpy (projection and distances accumulated in
    the kernel's order of dims); last_on_ties: the self-test's mutation"""
    nb, hid, T12 = lat.shape
    z = np.transpose(f32(lat), (0, 2, 1)).reshape(nb * T12, hid)
    codes = np.zeros((z.shape[0], nvalid), np.int64)
    for P, q0, q1 in ((f32(psem), 0, nsem), (f32(pac), nsem, nvalid)):
        r = np.zeros((z.shape[0], P.shape[0]), np.float32)
        for c in range(hid):
            r = f32(r + f32(z[:, c:c + 1] * P[None, :, c]))
        for q in range(q0, q1):
            E = f32(cbk[q])
            dist = np.zeros((z.shape[0], E.shape[0]), np.float32)
            for k0 in range(0, E.shape[1], 4):
                dd = f32(r[:, None, k0:k0 + 4] - E[None, :, k0:k0 + 4])
                sq = f32(dd * dd)
                dist = f32(dist + f32(f32(f32(sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]))
            idx = dist.shape[1] - 1 - np.argmin(dist[:, ::-1], 1) if last_on_ties else np.argmin(dist, 1)
            codes[:, q] = idx
            r = f32(r - E[idx])
    return codes
