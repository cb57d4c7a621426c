"""k_attn_tileh (qtts_hip_attn_tiled_bf16, the bf16 prefill attention precision)
against attn_ref.attend in float64 at its own edges -- tiles of BM = 64
positions, blocks of BN = 64 keys -- with test_gpu_attn_tile.py's inputs and
cases, and the switch end to end on that file's hd128 model.

The bound, derived for what the kernel rounds (u = 2^-8, half an ulp of bf16),
on the q the call left in place and the K / V the cache holds after it:

    ds_t  = c * sum_j |q_j| |k_tj| / sqrt(HD) + C_ABS                   (per key)
            c = 2u + u^2 + C_DOT  fp32 cache (q and K rounded), u + C_DOT  bf16 cache (K exact)
    bound = (expm1(2 max_t ds_t) + 2u + u_v + C_DOT) * sum_t p_t |v_td| + C_ABS
            u_v = u  fp32 cache (V rounded), 0  bf16 cache

2u: P rounded in the numerator and in the row sum (the kernel sums the rounded
P, so out is a convex combination of the V rows it multiplied); expm1 instead
of the first-order 2 ds because ds is no longer tiny.  The planted-key
assertions (weight >= 0.5, on the reference alone) are what makes this looser
bound still tell a dropped key, an extra key or a mask off by one.
Measured err / bound on an MI355X: DESIGN.md "The opt-in bf16 prefill attention".
"""
import numpy as np
import pytest

import qtts
import test_gpu_attn_tile as T
from attn_ref import C_ABS, C_DOT, attend, norm_rope, widen
from oracle_py import DEFAULT
from synth_model import prompt_ids

pytestmark = [pytest.mark.gpu]

BM, BN, S, ROWS = 64, 64, 192, 128
U = 2.0 ** -8


@pytest.fixture(autouse=True)
def _this_kernel(monkeypatch):
    """the helpers of test_gpu_attn_tile.py on a cache of 3 BN positions and the bf16 entry"""
    monkeypatch.setattr(T, "S", S)
    monkeypatch.setattr(qtts.Kernels, "attn_tiled", staticmethod(qtts.Kernels.attn_tiled_bf16))


def bound_bf16(q, K, V, P, cache_is_bf16):
    """the bound above: q [NH, HD], K / V [n, KV, HD] float64, P [NH, n] the reference's weights"""
    NH, HD = q.shape
    gph = NH // K.shape[1]
    c, u_v = (U + C_DOT, 0.0) if cache_is_bf16 else (2 * U + U * U + C_DOT, U)
    b = np.zeros((NH, HD))
    for h in range(NH):
        ds = c * (np.abs(K[:, h // gph]) @ np.abs(q[h])) / np.sqrt(HD) + C_ABS
        b[h] = (np.expm1(2 * ds.max()) + 2 * U + u_v + C_DOT) * (P[h] @ np.abs(V[:, h // gph])) + C_ABS
    return b


def check(path, I, segs, q=None, qn=None, kn=None, kbits=None, plant=None, above=None):
    """test_gpu_attn_tile.check_tiled's protocol (both cache types, NaN from each segment's first position on) under
    the bf16 bound, the reference on the device's own q rows"""
    NH, KV, HD, gph, AD = I.NH, I.KV, I.HD, I.NH // I.KV, I.NH * I.HD
    q, qn, kn = I.qkv if q is None else q, I.qn if qn is None else qn, I.kn if kn is None else kn
    kb0, vb0 = (I.kbits if kbits is None else kbits).copy(), I.vbits.copy()
    for b, p0, n in segs:
        kb0[b, p0:], vb0[b, p0:] = 0x7FC0, 0x7FC0
    for name, k0, v0, wide in (("fp32", widen(kb0), widen(vb0), lambda a: a), ("bf16", kb0, vb0, widen)):
        ran, out, q1, k1, v1 = T.dev_tiled(q, k0, v0, qn, kn, I.cos, I.sin, segs, NH, KV, HD)
        assert ran, "covered shape refused"
        worst, r = 0.0, 0
        for b, p0, n in segs:
            for p in range(p0, p0 + n):
                tag = f"{name} row {r} (slot {b}, pos {p})"
                K, V = (wide(c[b, :p + 2]).astype(np.float64).reshape(-1, KV, HD) for c in (k1, v1))
                assert np.isfinite(K[:p + 1]).all() and np.isfinite(V[:p + 1]).all(), "the test's own rows, " + tag
                qd = q1[r, :AD].reshape(NH, HD).astype(np.float64)
                ref, _, P = attend(qd, K[:p + 1], V[:p + 1])
                if plant and r in plant:
                    assert (P[::gph, plant[r]] >= 0.5).all(), f"planted key {plant[r]} weighs too little, {tag}"
                if above and r in above:
                    assert above[r] == p + 1 < p0 + n
                    assert (attend(qd, K, V)[2][::gph, p + 1] >= 0.5).all(), "key p + 1 too light, " + tag
                bound = bound_bf16(qd, K[:p + 1], V[:p + 1], P, name == "bf16")
                ratio = float((np.abs(out[r].reshape(NH, HD).astype(np.float64) - ref) / bound).max())
                assert ratio <= 1.0, f"{path} {tag}: err / bound {ratio:.3f}"   # (a NaN fails here too)
                worst, r = max(worst, ratio), r + 1
        print(f"err / bound  {path} {name}  {worst:.4f}")


@pytest.mark.parametrize("NH,KV,HD", T.SHAPES)
@pytest.mark.parametrize("segs", [[(0, 5, BM - 1), (1, BN + 3, BM + 1)], [(0, 0, 1), (1, BN, 1)]],
                         ids=["tile_edges", "one_row"])
def test_tiled_attention_bf16(gpu, NH, KV, HD, segs):
    check(f"k_attn_tileh HD{HD} gph{NH // KV}", T.Inputs(NH, KV, HD, rows=ROWS), segs)


def planted_case(NH, KV, HD):
    """test_gpu_attn_tile's planted-key case at BN = 64: slot 0 at positions 69 .. 133; the dominant key of 72 at
    key 0, of 73 at the last key of a full block, of 77 at the first key of its diagonal block, of 82 at its own
    position, and position 85's key, written by the same call, scores 12 against 84's query"""
    I = T.Inputs(NH, KV, HD, rows=ROWS)
    gph, AD, p0 = NH // KV, NH * HD, 69
    qn = (np.float32(T.plant_gain(HD)) * I.qn).astype(np.float32)
    q, kbits = I.qkv.copy(), I.kbits.copy()
    plant = {72 - p0: 0, 73 - p0: BN - 1, 77 - p0: BN, 82 - p0: 82}
    for r, ts in plant.items():
        qh = q[r, :AD].reshape(NH, HD)
        if ts == p0 + r:
            q[r, AD:AD + KV * HD] = (0.5 * qh[::gph]).ravel()
        else:
            q_hat = norm_rope(qh, qn, I.cos[p0 + r], I.sin[p0 + r])[0]
            for kvh in range(KV):
                kbits[0, ts, kvh * HD:(kvh + 1) * HD] = T.planted_row(q_hat[kvh * gph])
    r = 84 - p0
    q_hat = norm_rope(q[r, :AD].reshape(NH, HD)[::gph], qn, I.cos[84], I.sin[84])[0]
    q[r + 1, AD:AD + KV * HD] = (T.unrope(q_hat, I.cos[85], I.sin[85]) / qn).astype(np.float32).ravel()
    return I, [(0, p0, BM + 1), (1, 5, BM - 1)], dict(q=q, qn=qn, kn=qn, kbits=kbits, plant=plant, above={r: 85})


@pytest.mark.parametrize("NH,KV,HD", T.SHAPES)
def test_tiled_attention_bf16_planted_key(gpu, NH, KV, HD):
    I, segs, kw = planted_case(NH, KV, HD)
    check(f"k_attn_tileh HD{HD} gph{NH // KV} planted", I, segs, **kw)


@pytest.mark.parametrize("NH,KV,HD,win", [(4, 4, 32, 0), (8, 2, 64, 0), (4, 4, 64, 16)])
def test_tiled_attention_bf16_reports_shapes_it_does_not_cover(gpu, NH, KV, HD, win):
    """HD 32, four query heads per kv head and a window return 1: out, q and both caches keep their bits"""
    I = T.Inputs(NH, KV, HD)
    for k0, v0 in ((widen(I.kbits), widen(I.vbits)), (I.kbits, I.vbits)):
        ran, out, q1, k1, v1 = T.dev_tiled(I.qkv, k0, v0, I.qn, I.kn, I.cos, I.sin, [(0, 5, 40)], NH, KV, HD, win=win)
        assert not ran and np.isnan(out).all()
        for a, b in ((q1, I.qkv[:40]), (k1, k0), (v1, v0)):
            T._same(a, b, "q rows / K cache / V cache")


def _prefill(m, n):
    """(hidden, k_attn_tileh launches, k_attn_tile launches) of n seeded rows"""
    c0, e0 = qtts.Kernels.attn_tileh_launches(), qtts.Kernels.attn_tile_launches()
    h = m.prefill((np.random.default_rng(n).standard_normal((n, m.cfg.talker_hidden)) * 0.5).astype(np.float32))
    return h, qtts.Kernels.attn_tileh_launches() - c0, qtts.Kernels.attn_tile_launches() - e0


def test_switch_rows_and_determinism(gpu, monkeypatch):
    from conftest import model_dir
    monkeypatch.delenv("QTTS_HIP_PREFILL_ATTN", raising=False)
    plain, m = qtts.QwenTTS(model_dir("hd128")), qtts.QwenTTS(model_dir("hd128"))
    try:
        assert m.prefill_attention_precision() == qtts.PREFILL_ATTN_EXACT
        want = {n: _prefill(plain, n) for n in (300, 128)}     # a context that never called the setter
        assert want[300][1:] == (0, m.cfg.talker_layers) and want[128][1:] == (0, 0)
        m.set_prefill_attention_precision("bf16")
        h, new, old = _prefill(m, 300)
        assert (new, old) == (m.cfg.talker_layers, 0)
        assert np.isfinite(h).all() and h.tobytes() != want[300][0].tobytes()
        assert _prefill(m, 300)[0].tobytes() == h.tobytes()
        e = want[300][0].astype(np.float64)
        print(f"measured  300 rows, hidden bf16 attention against exact: |d| / |exact| = "
              f"{np.linalg.norm(h - e) / np.linalg.norm(e):.3e}, max |d| = {np.abs(h - e).max():.3e}")
        h, new, old = _prefill(m, 128)                         # below the threshold: row by row, exact
        assert (new, old) == (0, 0) and h.tobytes() == want[128][0].tobytes()
        with pytest.raises(ValueError):
            m.set_prefill_attention_precision(2)
        assert m.prefill_attention_precision() == qtts.PREFILL_ATTN_BF16
        m.set_prefill_attention_precision("exact")
        h, new, old = _prefill(m, 300)
        assert (new, old) == (0, m.cfg.talker_layers) and h.tobytes() == want[300][0].tobytes()
    finally:
        plain.close()
        m.close()


def test_env_sets_the_default(gpu, monkeypatch):
    from conftest import model_dir
    monkeypatch.setenv("QTTS_HIP_PREFILL_ATTN", "bf16")
    m = qtts.QwenTTS(model_dir("hd128"))
    try:
        assert m.prefill_attention_precision() == qtts.PREFILL_ATTN_BF16
        assert _prefill(m, 300)[1] == m.cfg.talker_layers
    finally:
        m.close()


def test_a_prefix_entry_is_served_only_in_its_own_mode(gpu, monkeypatch):
    from conftest import model_dir
    monkeypatch.delenv("QTTS_HIP_PREFILL_ATTN", raising=False)
    ins = np.random.default_rng(77).integers(1000, 100000, size=300).tolist()   # 300 prefix rows: the tiled path
    m = qtts.QwenTTS(model_dir("hd128"))

    def run():
        m.set_params(max_tokens=4096, fixed=2, seed=9, **DEFAULT)
        c0, p0 = m.prefix_counters(), qtts.Kernels.attn_tileh_launches()
        m.set_utterance_instruct([ins])
        assert m.generate(prompt_ids("short"), "aiden", "english") is not None
        hits = tuple(b - a for a, b in zip(c0, m.prefix_counters()))[:2]
        return hits, qtts.Kernels.attn_tileh_launches() - p0, m.last_codes()

    try:
        made = run()
        assert made[:2] == ((0, 1), 0)                         # computed in exact mode
        m.set_prefill_attention_precision("bf16")
        other = run()
        assert other[0] == (0, 1) and other[1] > 0             # not served: computed again, on k_attn_tileh
        again = run()
        assert again[:2] == ((1, 0), 0) and np.array_equal(again[2], other[2])   # its own entry is
        m.set_prefill_attention_precision("exact")
        back = run()
        assert back[:2] == ((1, 0), 0) and np.array_equal(back[2], made[2])      # and the exact entry is still there
    finally:
        m.close()
