"""The references, the error bounds and the fp32 restatements every
kernel-level test of the codec decoder's small kernels shares (k_codec.hip: the
kernels between the contractions and the multi-stream placement kernels;
test_gpu_codec_ops.py on the device, test_codec_op_ref.py on a CPU box;
codec_op_cases.py holds the inputs and the buffers).

References.  Plain numpy float64 from each operation's definition (the codec
decoder as oracle_py.py / qtts_oracle.c restate it): the RVQ dequantisation is
a table lookup and a sum followed by two 1x1 projections, the depthwise conv a
causal correlation over [history | new], LayerNorm / RMSNorm / rotate-half RoPE
as written in any textbook.  The placement kernels are Python loops over
(stream, row, column) that say where each element has to end up.

Two classes.

Bit-equal (uint32 views).  Pure moves (k_clamp(_ms), k_copy2d, k_ms_index,
k_hist_ms, k_kv_shift_ms, k_hist_reset_ms, k_ms_state_save / load, the V rows
and the untouched rows of k_rope_kv_ms) against the loops; the contract-off
kernels k_rvq_sum(_ms) and k_dwconv(_ms) against an fp32 numpy restatement in
the kernel's order (sequential adds, a rounded product, then a rounded add).
That restatement is itself held to the float64 reference in the CPU test:

    k_rvq_sum   semantic: 0 (one term); acoustic: C_DOT * sum_q |e_q|
    k_dwconv    C_DOT * (|b| + sum_k |w_k| |x_k|)

(at most 15 adds / 7 products and 7 adds of fp32, each 2^-24 relative: below
1e-6 of the absolute sum, inside C_DOT = 2e-6.)

Float64 bound, per output element, from xgemm_ref.py's constants only (C_DOT
2e-6 and C_ABS 1e-6 for an accumulated sum, EPS_OP 2e-7 for about three fp32
roundings):

    k_rvq_proj(_ms)  C_DOT * (sum |ps| |ss| + sum |pa| |as|) + 2 * C_ABS + EPS_OP * |out|
                     (two accumulated dot products and their fp32 sum)
    k_ln_t(_ms)      enc_kernel_ref.ln_rows_ref, imported: b_mean, d_v, d_inv
    k_rms_rows       ms = mean x^2 off by d_ms = C_DOT * ms + C_ABS; inv = 1 / sqrt(ms + eps)
                     off by d_inv = inv * d_ms / (2 (ms + eps)) (the derivative of
                     (ms + eps)^-1/2); |x w| * d_inv + EPS_OP * |y| (inv's own
                     division and square root and the two products)
    k_rope_rows, q and K rows of k_rope_kv_ms
                     enc_kernel_ref.rope_ref, imported: 2 * EPS_OP * (|a cs| + |b sn|)

Buffers (codec_op_cases.py): NaN everywhere an op may not read (left of the
margin beyond H, right of a row's length, the gaps between planes, RoPE table
rows past the last position a valid or pad row uses), SENTINEL (ISENT for
ints) everywhere it may not write, a tail behind every output included.  RVQ
codes cannot be NaN and the kernel maps an out-of-range code to entry 0, so
one codebook index (POISON) is kept out of every valid code, its codebook rows
are NaN and the code rows behind each stream's valid frames hold it: an
over-read shows as NaN in the sums.

MEASURED: the largest err / bound per bound-class kernel that
test_gpu_codec_ops.py printed on an MI355X.  A record; nothing asserts on it.

    k_rvq_proj 0.0310   k_rvq_proj_ms 0.0159   k_ln_t 0.1399   k_ln_t_ms 0.1159
    k_rms_rows 0.1527   k_rope_rows 0.2679     k_rope_kv_ms 0.2628 (q and K rows)

Every kernel of the bit-equal class equalled its reference bit for bit (ratio 0).
"""
import numpy as np

from enc_kernel_ref import ISENT, _rng, f32, ln_rows_ref, rope_ref     # noqa: F401  (shared with the cases)
from xgemm_ref import C_ABS, C_DOT, EPS_OP, SENTINEL                   # noqa: F401

MEASURED = {      # kernel -> largest err / bound on an MI355X
    "k_rvq_proj": 0.0310, "k_rvq_proj_ms": 0.0159, "k_ln_t": 0.1399, "k_ln_t_ms": 0.1159, "k_rms_rows": 0.1527,
    "k_rope_rows": 0.2679, "k_rope_kv_ms": 0.2628,
}

NANF = np.float32(np.nan)
INT_MAX = 2 ** 31 - 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within(name, got, ref, bound):
    """asserts finite and |got - ref| <= bound; returns the largest err / bound"""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), (name, "NaN / inf in the output: an over-read or a missing write")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    ratio = float(np.max(r)) if err.size else 0.0
    assert np.all(err <= bound), (name, ratio, np.argwhere(~(err <= bound))[:4])
    return ratio


# ------------------------------------------------------------------ RVQ
def rvq_rows(codes, coff, ldc, t0, T, tv):
    """[n * T][ldc] code rows of a push as the operation defines them: stream s
    reads frame t0 + t of its own codes, a pad row repeats the last valid frame"""
    rows = []
    for s in range(len(tv)):
        for t in range(T):
            f = t0 + min(t, tv[s] - 1)
            rows.append(codes[coff[s] + f * ldc: coff[s] + (f + 1) * ldc])
    return np.array(rows)


def rvq_sum_ref(rows, cb, Q):
    """rows [R][>= Q] int, cb [Q][CB][vq] -> float64 ss, as [vq][R] and their bounds"""
    CB = cb.shape[1]
    c = rows[:, :Q].astype(np.int64)
    c = np.where((c < 0) | (c >= CB), 0, c)
    e = cb.astype(np.float64)[np.arange(Q)[None, :], c]                  # [R][Q][vq]
    ss, ac = e[:, 0].T, e[:, 1:].sum(1).T
    return ss, ac, np.zeros_like(ss), C_DOT * np.abs(e[:, 1:]).sum(1).T


def rvq_sum_model(rows, cb, Q, mut=()):
    """fp32, the kernel's order: 0 + e0; 0 + e1 + ... in turn"""
    CB = cb.shape[1]
    c = rows[:, :Q].astype(np.int64)
    c = np.where((c < 0) | (c >= CB), 0, c)
    ss = f32(np.float32(0) + cb[0][c[:, 0]])
    ac = np.zeros_like(ss)
    for q in range(1, Q):
        ac = f32(ac + cb[q][c[:, q]])
    return np.ascontiguousarray(ss.T), np.ascontiguousarray(ac.T)


def rvq_proj_ref(ps, pa, ss, ac):
    ps, pa, ss, ac = (np.asarray(v, np.float64) for v in (ps, pa, ss, ac))
    out = ps @ ss + pa @ ac
    return out, C_DOT * (np.abs(ps) @ np.abs(ss) + np.abs(pa) @ np.abs(ac)) + 2 * C_ABS + EPS_OP * np.abs(out)


def _fma(a, b, c):
    return f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def wave_sum_model(v):
    """[64][...] lane values -> the butterfly sum over the lanes, fp32"""
    lanes = np.arange(64)
    for step in (1, 2, 4, 8, 16, 32):
        v = f32(v + v[lanes ^ step])
    return v[0]


def rvq_proj_model(ps, pa, ss, ac, mut=()):
    """one wave per output, lane l takes k = l, l + 64, ... by fma, butterfly sums, s1 + s2"""
    half, vq = ps.shape
    R = ss.shape[1]
    kmax = vq - vq % 64 if "lanes" in mut else vq
    s1 = np.zeros((64, half, R), np.float32)
    s2 = np.zeros((64, half, R), np.float32)
    for k in range(kmax):
        lane = k % 64
        s1[lane] = _fma(ps[:, k:k + 1], ss[k][None, :], s1[lane])
        s2[lane] = _fma(pa[:, k:k + 1], ac[k][None, :], s2[lane])
    a, b = wave_sum_model(s1), wave_sum_model(s2)
    return a if "s1_only" in mut else f32(a + b)


# ------------------------------------------------------------------ depthwise conv
def dwconv_ref(x, hist, w, b):
    """x [C][L], hist [C][K-1] or None (zeros), w [C][K], b [C] or None -> (y, bound)"""
    C, L = x.shape
    K = w.shape[1]
    h = np.zeros((C, K - 1)) if hist is None else np.asarray(hist, np.float64)
    xp = np.concatenate([h, np.asarray(x, np.float64)], 1)
    win = np.stack([xp[:, k:k + L] for k in range(K)], 1)                # [C][K][L]
    w64 = np.asarray(w, np.float64)
    b64 = np.zeros(C) if b is None else np.asarray(b, np.float64)
    y = b64[:, None] + (w64[:, :, None] * win).sum(1)
    return y, C_DOT * (np.abs(b64)[:, None] + (np.abs(w64)[:, :, None] * np.abs(win)).sum(1))


def dwconv_model(xbuf, col0, ldx, tmin, w, b, C, L, K, mut=()):
    """fp32 in the kernel's order on the flat plane xbuf (column 0 of row 0 at
    col0): acc = b; acc += w * x, product and sum each rounded"""
    if "margin" in mut and tmin == 0:
        tmin = -(K - 1)
    acc = np.zeros((C, L), np.float32) if b is None else np.repeat(f32(b)[:, None], L, 1)
    c, t = np.arange(C)[:, None], np.arange(L)[None, :]
    for k in range(1 if "tap0" in mut else 0, K):
        ti = t - (K - 1) + k
        v = xbuf[col0 + c * ldx + np.maximum(ti, tmin)]
        with np.errstate(invalid="ignore"):
            acc = np.where(ti >= tmin, f32(acc + f32(w[:, k:k + 1] * v)), acc)
    return acc


# ------------------------------------------------------------------ norms
def block_sum_model(v):
    """[C][...] per-channel terms, thread c % 256 adds its channels in turn, then
    the four waves' butterfly sums are added left to right"""
    C = v.shape[0]
    th = np.zeros((256,) + v.shape[1:], np.float32)
    for c0 in range(0, C, 256):
        blk = v[c0:c0 + 256]
        th[:blk.shape[0]] = f32(th[:blk.shape[0]] + blk)
    w = [wave_sum_model(th[i * 64:(i + 1) * 64]) for i in range(4)]
    return f32(f32(f32(w[0] + w[1]) + w[2]) + w[3])


def ln_t_model(x, w, b, eps, mut=()):
    """x [C][L] -> y [L][C], fp32 as k_ln_t: two passes, 1 / sqrt(var + eps)"""
    C = x.shape[0]
    mean = f32(block_sum_model(x) / np.float32(C))
    d = f32(x - mean[None, :])
    if "one_pass" in mut:
        var = f32(f32(block_sum_model(f32(x * x)) / np.float32(C)) - f32(mean * mean))
    else:
        var = f32(block_sum_model(f32(d * d)) / np.float32(C - 1 if "biased" in mut else C))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(np.float32(1) / np.sqrt(f32(var + (np.float32(0) if "no_eps" in mut else np.float32(eps)))))
        o = f32(f32(d * inv[None, :]) * w[:, None])
        return np.ascontiguousarray(f32(o + b[:, None]).T)


def rms_rows_ref(x, w, eps):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    ms = (x * x).mean(-1)
    inv = 1.0 / np.sqrt(ms + eps)
    d_inv = inv * (C_DOT * ms + C_ABS) / (2.0 * (ms + eps))
    y = x * inv[:, None] * w
    return y, np.abs(x * w) * d_inv[:, None] + EPS_OP * np.abs(y)


def rms_rows_model(x, w, eps, mut=()):
    D = x.shape[1]
    ss = block_sum_model(f32(x * x).T)
    e = np.float32(0) if "no_eps" in mut else np.float32(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(np.float32(1) / np.sqrt(f32(f32(ss / np.float32(D - 1 if "biased" in mut else D)) + e)))
        return f32(f32(x * inv[:, None]) * w[None, :])


# ------------------------------------------------------------------ RoPE
def rope_pos_ref(x, nh, hd, cs, sn, pos):
    """rows x [R][nh * hd] rotated by the table rows pos [R]: (out, bound) by enc_kernel_ref.rope_ref"""
    pos = np.asarray(pos)
    return rope_ref(x, nh, hd, x.shape[0], np.asarray(cs)[pos], np.asarray(sn)[pos])


def rope_model(x, nh, hd, cs, sn, pos, mut=()):
    """fp32 as the kernels (contraction allowed there; products rounded here)"""
    R, half = x.shape[0], hd // 2
    pos = np.asarray(pos) + (1 if "pos" in mut else 0)
    q = x.reshape(R, nh, hd)
    a, c = q[:, :, :half], q[:, :, half:]
    c1, s1 = cs[pos][:, None, :half], sn[pos][:, None, :half]
    c2, s2 = (c1, s1) if "swap" in mut else (cs[pos][:, None, half:], sn[pos][:, None, half:])
    lo = f32(f32(a * c1) - f32(c * s1))
    hi = f32(f32(c * c2) + f32(a * s2))
    return np.concatenate([lo, hi], -1).reshape(R, nh * hd)


def clamp_ref(v):
    """NaN passes, -0 stays -0, +-inf -> +-1"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v < -1, np.float32(-1), np.where(v > 1, np.float32(1), v)).astype(np.float32)
