"""The float64 attention reference and the absolute error bound every attention
kernel test shares (test_gpu_attn.py, test_gpu_kv_bf16.py), and the bf16
helpers of the cache tests.

The bound, per output element d of head h, in float64:

    ds_t  = 2e-6 * sum_j |q_j| |k_tj| / sqrt(HD) + 1e-6            (per key)
    bound = (2 * max_t ds_t + 2e-6) * sum_t p_t |v_td| + 1e-6

2e-6 / 1e-6 are the GEMV tests' constants (fp32 dot products of up to 8192
terms); the factor 2 on ds is the first-order softmax sensitivity to a score
error.  q is the float64 normalised and rotated query, K / V the values the
cache holds after the call (widened for bf16), so one bound serves both cache
types.  The constants are not to be loosened to make a kernel pass:
test_gpu_attn.py's sensitivity self-test fails when the bound stops telling a
dropped key, a key counted twice, a wrong scale, a wrong RoPE row or a window
edge off by one from the right answer.
"""
import numpy as np

EPS = 1e-6
THETA = 1000000.0
C_DOT, C_ABS = 2e-6, 1e-6


# ------------------------------------------------------------------ bf16 in numpy
def rne_bf16(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even -- the rule the
    cache writers state, restated here"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rope_tables(S, HD):
    half = HD // 2
    freq = (1.0 / np.power(np.float32(THETA), (2 * np.arange(half, dtype=np.float32)) / np.float32(HD))).astype(np.float32)
    ang = np.arange(S, dtype=np.float32)[:, None] * freq[None, :]
    c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    return np.concatenate([c, c], 1), np.concatenate([s, s], 1)


# ------------------------------------------------------------------ float64 reference
def norm_rope(x, w, cos_p, sin_p, eps=EPS):
    """per-head RMSNorm with weight w, then rotate-half RoPE with the table rows
    cos_p / sin_p, in float64.  x [..., HD].  Returns (y, mag): mag =
    |n_i c_i| + |n_partner s_i|, the magnitude the stored-row bound scales with"""
    x = np.asarray(x, np.float64)
    half = x.shape[-1] // 2
    n = x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps) * np.asarray(w, np.float64)
    c, s = np.asarray(cos_p, np.float64), np.asarray(sin_p, np.float64)
    partner = np.concatenate([n[..., half:], n[..., :half]], axis=-1)
    sign = np.concatenate([-np.ones(half), np.ones(half)])
    return n * c + sign * partner * s, np.abs(n * c) + np.abs(partner * s)


def stored_bound(mag):
    """|stored k (or in-place q) - float64 value|: about six fp32 roundings,
    3.6e-7 relative, with a 3x margin"""
    return 1e-6 * mag + 1e-7


def attend(q, K, V, scale=None, dup=None):
    """softmax(q K^T / sqrt(HD)) V in float64 with GQA: q [NH, HD], K / V
    [n, KV, HD] (the keys the row attends, in order).  Returns (out [NH, HD],
    bound [NH, HD], P [NH, n]).  scale / dup: the sensitivity self-test's
    mutations (another score scale; key index counted twice)."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    NH, HD = q.shape
    gph = NH // K.shape[1]
    if dup is not None:
        K, V = np.concatenate([K, K[dup:dup + 1]]), np.concatenate([V, V[dup:dup + 1]])
    sc = 1.0 / np.sqrt(HD) if scale is None else scale
    out, bound, P = np.zeros((NH, HD)), np.zeros((NH, HD)), np.zeros((NH, K.shape[0]))
    for h in range(NH):
        k, v = K[:, h // gph], V[:, h // gph]
        s = k @ q[h] * sc
        w = np.exp(s - s.max())
        p = w / w.sum()
        ds = C_DOT * (np.abs(k) @ np.abs(q[h])) / np.sqrt(HD) + C_ABS
        out[h] = p @ v
        bound[h] = (2 * ds.max() + C_DOT) * (p @ np.abs(v)) + C_ABS
        P[h] = p
    return out, bound, P


def window_lo(p, win):
    """first key of row p's window (win 0: none)"""
    return max(0, p + 1 - win) if win > 0 else 0
