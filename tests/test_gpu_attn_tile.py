"""k_attn_tile (qtts_hip_attn_tiled) against the float64 reference and bound of
attn_ref.py at its own edges: tiles of BM = 32 positions, blocks of BN = 32
keys.  Inputs as test_gpu_attn.py.  Measured err / bound: DESIGN.md section 4."""
import numpy as np
import pytest

import qtts
from attn_ref import EPS, attend, norm_rope, rne_bf16, rope_tables, stored_bound, widen

pytestmark = [pytest.mark.gpu]

BM, BN, S = 32, 32, 96
SHAPES = [(16, 8, 128), (4, 4, 64), (4, 2, 64)]


class Inputs:
    def __init__(self, NH, KV, HD, slots=2, rows=80):
        rng = np.random.default_rng(1000 * NH + 100 * KV + HD)
        self.NH, self.KV, self.HD = NH, KV, HD
        self.qkv = rng.standard_normal((rows, (NH + 2 * KV) * HD)).astype(np.float32)
        self.qn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.kn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.cos, self.sin = rope_tables(S, HD)
        self.kbits = rne_bf16(rng.standard_normal((slots, S, KV * HD)).astype(np.float32))
        self.vbits = rne_bf16(rng.standard_normal((slots, S, KV * HD)).astype(np.float32))


def plant_gain(HD): return max(1.0, float(np.sqrt(12.0 / np.sqrt(HD))))   # the token's own key scores 12


def planted_row(q_hat):   # c q_hat with c = 12 sqrt(HD) / |q_hat|^2, as bf16 bits
    q = np.asarray(q_hat, np.float64)
    return rne_bf16((12.0 * np.sqrt(q.shape[-1]) / (q @ q) * q).astype(np.float32))


def unrope(y, cos_p, sin_p):   # the rotate-half RoPE of norm_rope undone
    half = y.shape[-1] // 2
    partner = np.concatenate([y[..., half:], y[..., :half]], axis=-1)
    return y * cos_p - np.concatenate([-np.ones(half), np.ones(half)]) * partner * sin_p


def _same(a, b, msg):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


def dev_tiled(q, kc, vc, qn, kn, cos, sin, segs, NH, KV, HD, win=0):
    """attn_tiled, prep 1, over segs [(slot, pos0, count)]: (covered, out, q rows, kc, vc after the call)"""
    import torch
    t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to("cuda:0")
    back = lambda x, like: x.cpu().numpy().view(np.uint16) if like.dtype == np.uint16 else x.cpu().numpy()
    table, row0 = [], 0
    for b, p0, n in segs:
        table.append([b, row0, p0, n])
        row0 += n
    qd, kcd, vcd = t(q[:row0]), t(kc), t(vc)
    out = torch.full((row0, NH * HD), float("nan"), dtype=torch.float32, device="cuda:0")
    ran = qtts.Kernels.attn_tiled(out, qd, q.shape[1], kcd, vcd, t(qn), t(kn), t(cos), t(sin),
                                  t(np.asarray(table, np.int32)), len(segs), NH, KV, HD, kc.shape[1], kc.shape[0], row0,
                                  EPS, win, 1 if kc.dtype == np.uint16 else 0, 1)
    torch.cuda.synchronize()
    return ran, out.cpu().numpy(), qd.cpu().numpy(), back(kcd, kc), back(vcd, vc)


def check_tiled(path, I, segs, q=None, qn=None, kn=None, kbits=None, plant=None, above=None):
    """check_prep of test_gpu_attn.py on both cache types: slots filled below their segment's first position, NaN
    from there on (a read past a row's keys shows).  plant {row: key}: the key weighs >= 0.5 in the reference;
    above {row: p + 1}: a reference that took that key would give it >= 0.5."""
    NH, KV, HD, gph, AD = I.NH, I.KV, I.HD, I.NH // I.KV, I.NH * I.HD
    q = I.qkv if q is None else q
    qn, kn = I.qn if qn is None else qn, I.kn if kn is None else kn
    kb0, vb0 = (I.kbits if kbits is None else kbits).copy(), I.vbits.copy()
    for b, p0, n in segs:
        kb0[b, p0:], vb0[b, p0:] = 0x7FC0, 0x7FC0
    k32 = None
    for name, k0, v0, wide in (("fp32", widen(kb0), widen(vb0), lambda a: a), ("bf16", kb0, vb0, widen)):
        ran, out, q1, k1, v1 = dev_tiled(q, k0, v0, qn, kn, I.cos, I.sin, segs, NH, KV, HD)
        assert ran, "covered shape refused"
        written, worst, r = np.zeros(k0.shape[:2], bool), 0.0, 0
        for b, p0, n in segs:
            for p in range(p0, p0 + n):
                tag = f"{name} row {r} (slot {b}, pos {p})"
                qh, k, v = q[r, :AD].reshape(NH, HD), q[r, AD:AD + KV * HD].reshape(KV, HD), q[r, AD + KV * HD:]
                q_hat, qmag = norm_rope(qh, qn, I.cos[p], I.sin[p])
                k_hat, kmag = norm_rope(k, kn, I.cos[p], I.sin[p])
                written[b, p] = True
                assert (np.abs(q1[r, :AD] - q_hat.ravel()) <= stored_bound(qmag.ravel())).all(), "q in place, " + tag
                _same(q1[r, AD:], q[r, AD:], "k | v of the row, " + tag)
                if name == "fp32":
                    assert (np.abs(k1[b, p] - k_hat.ravel()) <= stored_bound(kmag.ravel())).all(), "stored k, " + tag
                    _same(v1[b, p], v, "stored v, " + tag)
                else:
                    _same(k1[b, p], rne_bf16(k32[b, p]), "stored k bf16, " + tag)
                    _same(v1[b, p], rne_bf16(v), "stored v bf16, " + tag)
                K, V = (wide(c[b, :p + 2]).astype(np.float64).reshape(-1, KV, HD) for c in (k1, v1))
                assert np.isfinite(K[:p + 1]).all() and np.isfinite(V[:p + 1]).all(), "the test's own rows, " + tag
                ref, bound, P = attend(q_hat, K[:p + 1], V[:p + 1])
                if plant and r in plant:
                    assert (P[::gph, plant[r]] >= 0.5).all(), f"planted key {plant[r]} weighs too little, {tag}"
                if above and r in above:
                    assert above[r] == p + 1 < p0 + n
                    assert (attend(q_hat, K, V)[2][::gph, p + 1] >= 0.5).all(), "key p + 1 too light, " + tag
                ratio = float((np.abs(out[r].reshape(NH, HD).astype(np.float64) - ref) / bound).max())
                assert ratio <= 1.0, f"{path} {tag}: err / bound {ratio:.3f}"   # (a NaN fails here too)
                worst, r = max(worst, ratio), r + 1
        _same(k1[~written], k0[~written], name + " other K rows")
        _same(v1[~written], v0[~written], name + " other V rows")
        print(f"err / bound  {path} {name}  {worst:.4f}")
        k32 = k1 if k32 is None else k32


@pytest.mark.parametrize("NH,KV,HD", SHAPES)
@pytest.mark.parametrize("segs", [[(0, 5, BM - 1), (1, BN + 3, BM + 1)], [(0, 0, 1), (1, BN, 1)]],
                         ids=["tile_edges", "one_row"])
def test_tiled_attention(gpu, NH, KV, HD, segs):
    """a segment one row short of a tile from position 5 and one a row longer from BN + 3 (two tiles, three key
    blocks); a single row at position 0, and one at BN (one full block and the diagonal element)"""
    check_tiled(f"k_attn_tile HD{HD} gph{NH // KV}", Inputs(NH, KV, HD), segs)


@pytest.mark.parametrize("NH,KV,HD", SHAPES)
def test_tiled_attention_planted_key(gpu, NH, KV, HD):
    """slot 0 at positions 37 .. 69: the dominant key of 40 at key 0, of 41 at the last key of a full block, of 45
    at the first key of its diagonal block, of 50 at its own position (raw k = raw q halved, kn_w = qn_w), and
    position 53's key, written by the same call, scores 12 against 52's query: only the causal mask keeps it out"""
    I = Inputs(NH, KV, HD)
    gph, AD, p0 = NH // KV, NH * HD, 37
    qn = (np.float32(plant_gain(HD)) * I.qn).astype(np.float32)
    q, kbits = I.qkv.copy(), I.kbits.copy()
    plant = {40 - p0: 0, 41 - p0: BN - 1, 45 - p0: BN, 50 - p0: 50}
    for r, ts in plant.items():
        qh = q[r, :AD].reshape(NH, HD)
        if ts == p0 + r:
            q[r, AD:AD + KV * HD] = (0.5 * qh[::gph]).ravel()
        else:
            q_hat = norm_rope(qh, qn, I.cos[p0 + r], I.sin[p0 + r])[0]
            for kvh in range(KV):
                kbits[0, ts, kvh * HD:(kvh + 1) * HD] = planted_row(q_hat[kvh * gph])
    r = 52 - p0
    q_hat = norm_rope(q[r, :AD].reshape(NH, HD)[::gph], qn, I.cos[52], I.sin[52])[0]
    q[r + 1, AD:AD + KV * HD] = (unrope(q_hat, I.cos[53], I.sin[53]) / qn).astype(np.float32).ravel()
    check_tiled(f"k_attn_tile HD{HD} gph{gph} planted", I, [(0, p0, BM + 1), (1, 5, BM - 1)], q=q, qn=qn, kn=qn,
                kbits=kbits, plant=plant, above={r: 53})


@pytest.mark.parametrize("NH,KV,HD,win", [(4, 4, 32, 0), (8, 2, 64, 0), (4, 4, 64, 16)])
def test_tiled_attention_reports_shapes_it_does_not_cover(gpu, NH, KV, HD, win):
    """HD 32, four query heads per kv head and a window return 1: out, q and both caches keep their bits"""
    I = Inputs(NH, KV, HD)
    for k0, v0 in ((widen(I.kbits), widen(I.vbits)), (I.kbits, I.vbits)):
        ran, out, q1, k1, v1 = dev_tiled(I.qkv, k0, v0, I.qn, I.kn, I.cos, I.sin, [(0, 5, 40)], NH, KV, HD, win=win)
        assert not ran and np.isnan(out).all()
        for a, b in ((q1, I.qkv[:40]), (k1, k0), (v1, v0)):
            _same(a, b, "q rows / K cache / V cache")


def test_talker_prefill_takes_the_tiled_path_from_256_rows(gpu, monkeypatch):
    """the hd128 model of test_gpu_long.py: 300 rows take the tiled launch, 128 do not, nor does a model created
    with QTTS_HIP_ATTN_TILE=0, whose 300-row hidden agrees under test_prefill_gemm_matches_round5_gemm's bar"""
    from conftest import model_dir
    hid, moved, VAR = {}, {}, "QTTS_HIP_ATTN_TILE"
    for env in (None, "0"):
        monkeypatch.setenv(VAR, env) if env else monkeypatch.delenv(VAR, raising=False)
        m = qtts.QwenTTS(model_dir("hd128"))
        try:
            for n in (300, 128):
                e = np.random.default_rng(n).standard_normal((n, m.cfg.talker_hidden)) * 0.5
                c0 = qtts.Kernels.attn_tile_launches()
                hid[env, n] = m.prefill(e.astype(np.float32))
                moved[env, n] = qtts.Kernels.attn_tile_launches() - c0
        finally:
            m.close()
    assert moved[None, 300] > 0 and moved[None, 128] == 0 and moved["0", 300] == 0 and moved["0", 128] == 0, moved
    np.testing.assert_allclose(hid[None, 300], hid["0", 300], atol=1e-4, rtol=1e-4)
    _same(hid[None, 128], hid["0", 128], "128 rows: the same kernels, the same bits")
