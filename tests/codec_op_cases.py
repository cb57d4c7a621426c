"""The cases of the codec decoder's small kernels (codec_op_ref.py has the
references, the bounds and the rules for the buffers): the smallest shapes
that reach every trip count and branch of each kernel.

A Case holds one launch of qtts_hip_codec_op: the operands as host arrays (inp
entries: None, an array, (array, offset in elements), ("out", j, offset): the
output buffer j, or ("ptrs", [(j, offset), ...]): a device table of pointers
into output buffers), the outputs prefilled, n / s / eps, `model` (the kernel's
arithmetic restated in fp32 numpy on copies of the outputs; mut: a deliberate
defect) and `check` (asserts the outputs after a launch, returns the largest
err / bound; 0 for the bit-equal class).  twin: the single-plane launch an
n = 1 multi-stream case must equal bit for bit, with `twin_same`."""
from dataclasses import dataclass, field

import numpy as np

import codec_op_ref as R
import qtts
from codec_op_ref import INT_MAX, ISENT, NANF, SENTINEL, _rng, f32, same

TAIL = 9            # sentinel elements behind every output
LM, RM = 64, 5      # NaN columns left (the margin lives in its last H) and right of a channel-major row


@dataclass
class Case:
    kernel: str
    name: str
    op: int
    inp: list
    out: list
    n: tuple
    s: tuple = ()
    eps: float = 0.0
    model: object = None
    check: object = None
    twin: object = None
    twin_same: object = None
    muts: tuple = ()          # the defects this kernel's model knows
    meta: dict = field(default_factory=dict)

    def id(self):
        return f"{self.kernel}-{self.name}"

    def run_model(self, mut=()):
        outs = [np.array(o[0] if isinstance(o, tuple) else o) for o in self.out]
        self.model(outs, mut)
        return outs


def sent(shape, dtype=np.float32):
    return np.full(shape, ISENT if dtype == np.int32 else SENTINEL, dtype)


def with_tail(a, tail=TAIL):
    return np.concatenate([np.asarray(a).reshape(-1), sent(tail, a.dtype)])


# ------------------------------------------------------------------ RVQ
POISON = 5           # the codebook index no valid code takes; its rows are NaN


def rvq_inputs(vq, Q, CB, frames, seed):
    rng = _rng("rvq", vq, Q, CB, frames, seed)
    cb = rng.standard_normal((Q, CB, vq)).astype(np.float32)
    cb[:, POISON] = NANF
    codes = rng.integers(0, CB - 1, (frames, Q)).astype(np.int32)
    codes[codes >= POISON] += 1
    special = [-1, CB, INT_MAX, -INT_MAX - 1, CB + 7]       # all of them read entry 0
    for i, v in enumerate(special):
        codes[i % frames, (i * 3) % Q] = v
    return cb, codes


def rvq_sum_case(vq, Q, T, ms=None, CB=12, seed=0):
    """ms: None (k_rvq_sum) or (t0, tv tuple): n streams, codes rows of ldc = Q + 2 ints"""
    if ms is None:
        cb, codes = rvq_inputs(vq, Q, CB, T, seed)
        rows = codes
        inp = [with_tail(codes, 0), cb.reshape(-1)]
        n_arg, op, R_ = (T, Q, CB, vq), qtts.CO_RVQ_SUM, T
        name = f"vq{vq}-Q{Q}-T{T}"
    else:
        t0, tv = ms
        n, ldc = len(tv), Q + 2
        # streams laid out in the order (1, 2, 0, ...): coff is not monotone in s
        order = list(range(1, n)) + [0]
        flat, coff, pos = [], [0] * n, 0
        for s in order:
            cb, codes = rvq_inputs(vq, Q, CB, t0 + tv[s], seed + s)
            blk = np.full((t0 + tv[s] + 2, ldc), POISON, np.int32)        # two poisoned frames behind the valid ones
            blk[:t0 + tv[s], :Q] = codes
            coff[s] = pos
            flat.append(blk.reshape(-1))
            pos += blk.size
        cb = rvq_inputs(vq, Q, CB, 1, seed)[0]
        flat = np.concatenate(flat)
        rows = R.rvq_rows(flat, coff, ldc, t0, T, tv)
        inp = [flat, np.array(coff, np.int64), cb.reshape(-1), np.array(tv, np.int32)]
        n_arg, op, R_ = (ldc, t0, T, n, Q, CB, vq), qtts.CO_RVQ_SUM_MS, n * T
        name = f"vq{vq}-Q{Q}-T{T}-t0.{t0}-tv{'.'.join(map(str, tv))}"
    ss64, ac64, b_s, b_a = R.rvq_sum_ref(rows, cb, Q)
    ss32, ac32 = R.rvq_sum_model(rows, cb, Q)
    # the fp32 restatement is inside the float64 bound; the device must equal it bit for bit
    R.within("rvq_sum restatement", ss32, ss64, b_s)
    R.within("rvq_sum restatement", ac32, ac64, b_a)
    if Q == 1:
        assert not ac32.any()

    def model(outs, mut):
        outs[0][:vq * R_], outs[1][:vq * R_] = ss32.reshape(-1), ac32.reshape(-1)

    def check(outs):
        assert np.all(np.isfinite(outs[0][:vq * R_])) and np.all(np.isfinite(outs[1][:vq * R_])), "a poisoned code was read"
        assert same(outs[0], with_tail(ss32)) and same(outs[1], with_tail(ac32))
        return 0.0
    kern = "k_rvq_sum" if ms is None else "k_rvq_sum_ms"
    return Case(kern, name, op, inp, [sent(vq * R_ + TAIL), sent(vq * R_ + TAIL)], n_arg, model=model, check=check,
                meta=dict(ss=ss32, ac=ac32))


def rvq_proj_case(vq, half, T, n=0, seed=0):
    """n 0: k_rvq_proj; n >= 1: k_rvq_proj_ms with n planes"""
    rng = _rng("rvq-proj", vq, half, T, n, seed)
    Rr = max(n, 1) * T
    ps = (rng.standard_normal((half, vq)) / np.sqrt(vq)).astype(np.float32)
    pa = (rng.standard_normal((half, vq)) / np.sqrt(vq)).astype(np.float32)
    ss = rng.standard_normal((vq, Rr)).astype(np.float32)
    ac = (3 * rng.standard_normal((vq, Rr))).astype(np.float32)
    ref, bound = R.rvq_proj_ref(ps, pa, ss, ac)
    ldo = T + 3
    seg = 2 * half * ldo + 11                      # (the model's plane holds ccbdim = 2 * half rows)
    planes = max(n, 1)
    size = (planes - 1) * seg + half * ldo
    idx = (np.arange(planes)[None, :, None] * seg + np.arange(half)[:, None, None] * ldo
           + np.arange(T)[None, None, :]).reshape(half, Rr)
    out0 = sent(size + TAIL)

    def model(outs, mut):
        outs[0][idx] = R.rvq_proj_model(ps, pa, ss, ac, mut)

    def check(outs):
        ratio = R.within("rvq_proj", outs[0][idx], ref, bound)
        keep = np.ones(out0.shape, bool)
        keep[idx] = False
        assert same(outs[0][keep], out0[keep]), "a stray write"
        return ratio
    inp = [ps.reshape(-1), pa.reshape(-1), with_tail(ss, 0), with_tail(ac, 0)]
    if n == 0:
        return Case("k_rvq_proj", f"vq{vq}-half{half}-T{T}", qtts.CO_RVQ_PROJ, inp, [out0], (vq, half, T, ldo),
                    model=model, check=check, muts=("lanes", "s1_only"))
    return Case("k_rvq_proj_ms", f"vq{vq}-half{half}-T{T}-n{n}", qtts.CO_RVQ_PROJ_MS, inp, [out0],
                (vq, half, T, n, ldo), (seg,), model=model, check=check, muts=("lanes", "s1_only"))


# ------------------------------------------------------------------ depthwise conv
def dwconv_case(C, L, K, hist, bias, n=0, seed=0):
    """hist: the margin holds K - 1 history columns (tmin = -(K - 1)), else tmin = 0
    and the margin is NaN.  n 0: k_dwconv; n >= 1: k_dwconv_ms"""
    rng = _rng("dwconv", C, L, K, hist, bias, n, seed)
    planes, H = max(n, 1), (K - 1 if hist else 0)
    ldx, ldy = LM + L + RM, L + 3
    segx, segy = C * ldx + 13, C * ldy + 6
    xb = np.full(planes * segx, NANF, np.float32)
    w = rng.standard_normal((C, K)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32) if bias else None
    y0 = sent((planes - 1) * segy + C * ldy + TAIL)
    refs, idxs = [], []
    for p in range(planes):
        x = rng.standard_normal((C, L)).astype(np.float32)
        h = rng.standard_normal((C, H)).astype(np.float32) if H else None
        v = xb[p * segx:p * segx + C * ldx].reshape(C, ldx)
        v[:, LM:LM + L] = x
        if H:
            v[:, LM - H:LM] = h
        refs.append(R.dwconv_ref(x, h, w, b))
        idxs.append(p * segy + np.arange(C)[:, None] * ldy + np.arange(L)[None, :])

    def run(mut=()):
        return [R.dwconv_model(xb, p * segx + LM, ldx, -H, w, b, C, L, K, mut) for p in range(planes)]
    exact = run()
    for p in range(planes):
        R.within("dwconv restatement", exact[p], *refs[p])

    def model(outs, mut):
        for p, y in enumerate(run(mut)):
            outs[0][idxs[p]] = y

    def check(outs):
        keep = np.ones(y0.shape, bool)
        for p in range(planes):
            got = outs[0][idxs[p]]
            assert np.all(np.isfinite(got)), "NaN in the output: a read outside [history | new]"
            assert same(got, exact[p]), (p, float(np.nanmax(np.abs(got - exact[p]))))
            keep[idxs[p]] = False
        assert same(outs[0][keep], y0[keep]), "a stray write"
        return 0.0
    inp = [(xb, LM), w.reshape(-1), b]
    name = f"C{C}-L{L}-K{K}-{'hist' if hist else 'zero'}-{'b' if bias else 'nob'}"
    muts = ("tap0", "margin")
    if n == 0:
        return Case("k_dwconv", name, qtts.CO_DWCONV, inp, [y0], (ldx, H, C, L, K, ldy), model=model, check=check,
                    muts=muts)
    return Case("k_dwconv_ms", f"{name}-n{n}", qtts.CO_DWCONV_MS, inp, [y0], (ldx, H, C, L, K, ldy, n), (segx, segy),
                model=model, check=check, muts=muts)


# ------------------------------------------------------------------ norms
def norm_rows(rng, rows, D):
    """rows x [rows][D] cycling through: standard normal; mean 100, std 0.01 (a
    one-pass variance fails); constant (variance 0); mixed magnitudes across
    channels; small (mean square near eps); zero"""
    x = np.zeros((rows, D), np.float32)
    for r in range(rows):
        kind = r % 6
        g = rng.standard_normal(D)
        x[r] = [g, 100.0 + 0.01 * g, np.full(D, 3.25), g * 10.0 ** rng.integers(-3, 4, D), 1e-3 * g, np.zeros(D)][kind]
    return x


def ln_t_case(C, L, n=0, eps=1e-6, seed=0):
    rng = _rng("ln_t", C, L, n, seed)
    planes = max(n, 1)
    ldx = L + 3
    segx = C * ldx + 7
    xb = np.full(planes * segx, NANF, np.float32)
    w = rng.uniform(0.5, 1.5, C).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    xs = []
    for p in range(planes):
        x = np.ascontiguousarray(norm_rows(rng, L, C).T)                 # [C][L]: column t is one LayerNorm
        xb[p * segx:p * segx + C * ldx].reshape(C, ldx)[:, :L] = x
        xs.append(x)
    e32 = np.float32(eps)
    ref, bound = ln_rows_ref_t(xs, w, b, np.float64(e32))
    y0 = sent(planes * L * C + TAIL)

    def model(outs, mut):
        outs[0][:planes * L * C] = np.concatenate([R.ln_t_model(x, w, b, e32, mut) for x in xs]).reshape(-1)

    def check(outs):
        assert same(outs[0][planes * L * C:], y0[planes * L * C:]), "a stray write"
        return R.within("ln_t", outs[0][:planes * L * C].reshape(planes * L, C), ref, bound)
    inp = [xb, with_tail(w, 0), with_tail(b, 0)]
    muts = ("one_pass", "no_eps", "biased")
    if n == 0:
        return Case("k_ln_t", f"C{C}-L{L}", qtts.CO_LN_T, inp, [y0], (ldx, L, C), eps=float(e32), model=model,
                    check=check, muts=muts)
    return Case("k_ln_t_ms", f"C{C}-L{L}-n{n}", qtts.CO_LN_T_MS, inp, [y0], (ldx, L, C, n), (segx,), eps=float(e32),
                model=model, check=check, muts=muts)


def ln_rows_ref_t(xs, w, b, eps):
    refs = [R.ln_rows_ref(x.T, w, b, eps) for x in xs]
    return np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])


def rms_rows_case(M, D, eps=1e-5, seed=0):
    rng = _rng("rms", M, D, seed)
    x = norm_rows(rng, M, D)
    w = rng.uniform(0.5, 1.5, D).astype(np.float32)
    e32 = np.float32(eps)
    ref, bound = R.rms_rows_ref(x, w, np.float64(e32))
    y0 = sent(M * D + TAIL)

    def model(outs, mut):
        outs[0][:M * D] = R.rms_rows_model(x, w, e32, mut).reshape(-1)

    def check(outs):
        assert same(outs[0][M * D:], y0[M * D:]), "a stray write"
        return R.within("rms_rows", outs[0][:M * D].reshape(M, D), ref, bound)
    return Case("k_rms_rows", f"M{M}-D{D}", qtts.CO_RMS_ROWS, [with_tail(np.concatenate([x.reshape(-1)]), 0), w], [y0],
                (M, D), eps=float(e32), model=model, check=check, muts=("no_eps", "biased"))


# ------------------------------------------------------------------ RoPE
def rope_table(rows, hd, nan_from):
    """real angles; the upper half is perturbed so that cos[e] != cos[e + half];
    rows >= nan_from are NaN (no valid or pad row may use them)"""
    half = hd // 2
    ang = np.arange(rows)[:, None] * (10000.0 ** (-np.arange(half) / half))[None, :]
    cs = np.concatenate([np.cos(ang), np.cos(ang + 0.01)], 1).astype(np.float32)
    sn = np.concatenate([np.sin(ang), np.sin(ang + 0.01)], 1).astype(np.float32)
    assert np.any(cs[:, :half] != cs[:, half:])
    cs[nan_from:], sn[nan_from:] = NANF, NANF
    return cs, sn


def rope_rows_case(nh, hd, T, row0=130, seed=0):
    """the table pointer starts at row0, as a stream past its first pass hands it over"""
    rng = _rng("rope", nh, hd, T, seed)
    cs, sn = rope_table(row0 + T + 2, hd, row0 + T)
    x = rng.standard_normal((T, nh * hd)).astype(np.float32)
    ld = nh * hd + 4
    x0 = sent((T, ld))
    x0[:, :nh * hd] = x
    x0 = with_tail(x0)
    pos = row0 + np.arange(T)
    ref, bound = R.rope_pos_ref(x, nh, hd, cs, sn, pos)
    idx = np.arange(T)[:, None] * ld + np.arange(nh * hd)[None, :]

    def model(outs, mut):
        outs[0][idx] = R.rope_model(x, nh, hd, cs, sn, pos, mut)

    def check(outs):
        keep = np.ones(x0.shape, bool)
        keep[idx] = False
        assert same(outs[0][keep], x0[keep]), "a stray write"
        return R.within("rope_rows", outs[0][idx], ref, bound)
    return Case("k_rope_rows", f"nh{nh}-hd{hd}-T{T}", qtts.CO_ROPE_ROWS, [(cs.reshape(-1), row0 * hd),
                                                                        (sn.reshape(-1), row0 * hd)],
                [x0], (T, ld, nh, hd), model=model, check=check, muts=("swap", "pos"))


def rope_kv_case(nh, nkv, hd, T, sid, pos0, hl, tv, ns, S, seed=0):
    rng = _rng("rope-kv", nh, nkv, hd, T, sid, pos0, hl, tv, seed)
    n, hid, kvd = len(sid), nh * hd, nkv * hd
    last = max(p + T for p in pos0)                           # a pad row rotates too
    cs, sn = rope_table(last + 2, hd, last)
    q = rng.standard_normal((n * T, hid)).astype(np.float32)
    k = rng.standard_normal((n * T, kvd)).astype(np.float32)
    v = rng.standard_normal((n * T, kvd)).astype(np.float32)
    rowpos = np.array([pos0[s] + t for s in range(n) for t in range(T)])
    qref, qb = R.rope_pos_ref(q, nh, hd, cs, sn, rowpos)
    kref, kb = R.rope_pos_ref(k, nkv, hd, cs, sn, rowpos)
    q0, c0 = with_tail(q), sent(ns * S * kvd + TAIL)
    valid = [(s, t) for s in range(n) for t in range(T) if t < tv[s]]
    dst = np.array([sid[s] * S + hl[s] + t for s, t in valid])
    src = np.array([s * T + t for s, t in valid])
    assert len(set(dst)) == len(dst) and max(dst) < ns * S
    cidx = dst[:, None] * kvd + np.arange(kvd)[None, :]

    def model(outs, mut):
        outs[0][:q.size] = R.rope_model(q, nh, hd, cs, sn, rowpos, mut).reshape(-1)
        km = R.rope_model(k, nkv, hd, cs, sn, rowpos, mut)
        for s in range(n):
            for t in range(T):
                if t < tv[s] or "pad_store" in mut:
                    row = ((s if "sid" in mut else sid[s]) * S + hl[s] + t) * kvd
                    outs[1][row:row + kvd] = km[s * T + t]
                    outs[2][row:row + kvd] = v[s * T + t]

    def check(outs):
        assert same(outs[0][q.size:], q0[q.size:])
        keep = np.ones(c0.shape, bool)
        keep[cidx] = False
        assert same(outs[1][keep], c0[keep]) and same(outs[2][keep], c0[keep]), "a K / V row where none belongs"
        assert same(outs[2][cidx], v[src]), "V rows are moved, not computed"
        r1 = R.within("rope_kv q", outs[0][:q.size].reshape(q.shape), qref, qb)
        return max(r1, R.within("rope_kv k", outs[1][cidx], kref[src], kb[src]))
    ints = [np.array(a, np.int32) for a in (sid, pos0, hl, tv)]
    name = f"nh{nh}-nkv{nkv}-hd{hd}-T{T}-n{n}-tv{'.'.join(map(str, tv))}"
    return Case("k_rope_kv_ms", name, qtts.CO_ROPE_KV_MS, [with_tail(k, 0), with_tail(v, 0), cs.reshape(-1),
                                                          sn.reshape(-1)] + ints,
                [q0, c0.copy(), c0.copy()], (hid, nh, kvd, nkv, hd, T, n, S), model=model, check=check,
                muts=("swap", "pos", "pad_store", "sid"), meta=dict(q=q, k=k, kvd=kvd, hid=hid))


def rope_twin_case(nh, nkv, hd, T):
    """n = 1, sid (0), position 0: q and the K rows equal k_rope_rows bit for bit"""
    c = rope_kv_case(nh, nkv, hd, T, (0,), (0,), (0,), (T,), 1, T, seed=7)
    cs, sn = c.inp[2], c.inp[3]
    q = c.meta["q"]
    tq = Case("k_rope_rows", "twin-q", qtts.CO_ROPE_ROWS, [cs, sn], [with_tail(q)], (T, nh * hd, nh, hd),
              model=lambda outs, mut: outs[0].__setitem__(slice(0, q.size), R.rope_model(
                  q, nh, hd, cs.reshape(-1, hd), sn.reshape(-1, hd), np.arange(T)).reshape(-1)),
              check=lambda outs: 0.0)
    c.twin = tq
    c.twin_same = lambda mine, other: same(mine[0], other[0])
    c.name = "twin-" + c.name
    return c


# ------------------------------------------------------------------ index, clamp, copy
def ms_index_case(sid, hl, T):
    n = len(sid)
    rb = np.array([sid[s] for s in range(n) for t in range(T)], np.int32)
    pos = np.array([hl[s] + t for s in range(n) for t in range(T)], np.int32)

    def model(outs, mut):
        outs[0][:n * T] = np.repeat(np.arange(n), T) if "sid" in mut else rb
        outs[1][:n * T] = pos

    def check(outs):
        assert same(outs[0], with_tail(rb)) and same(outs[1], with_tail(pos))
        return 0.0
    return Case("k_ms_index", f"n{n}-T{T}", qtts.CO_MS_INDEX, [np.array(sid, np.int32), np.array(hl, np.int32)],
                [sent(n * T + TAIL, np.int32), sent(n * T + TAIL, np.int32)], (n, T), model=model, check=check,
                muts=("sid",))


def clamp_values(rng, n):
    one = np.float32(1)
    edge = [1e30, 1, -1, np.nextafter(one, np.float32(2)), -np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)),
            0.0, -0.0, np.inf, -np.inf, np.nan, -1e30, 1e-40]
    v = (2 * rng.standard_normal(n)).astype(np.float32)
    v[:len(edge)] = np.array(edge, np.float32)[:n]
    return v


def clamp_case(n):
    v = clamp_values(_rng("clamp", n), n)
    want = with_tail(R.clamp_ref(v))

    def model(outs, mut):
        outs[0][:n] = R.clamp_ref(outs[0][:n])
    return Case("k_clamp", f"n{n}", qtts.CO_CLAMP, [], [with_tail(v)], (n,), model=model,
                check=lambda outs: float(not same(outs[0], want) and _fail("clamp")))


def _fail(what):
    raise AssertionError(what)


def clamp_ms_case(T, spf, tv):
    n, L = len(tv), T * spf
    seg = LM + L + RM
    x = np.full(n * seg, NANF, np.float32)
    y0 = sent(n * L + TAIL)
    want = y0.copy()
    rng = _rng("clamp-ms", T, spf, tv)
    for s in range(n):
        x[s * seg:s * seg + L] = clamp_values(rng, L)          # (the padding holds finite samples too: none may be written)
        want[s * L:s * L + tv[s] * spf] = R.clamp_ref(x[s * seg:s * seg + tv[s] * spf])

    def model(outs, mut):
        for s in range(n):
            m = L if "all" in mut else tv[s] * spf
            outs[0][s * L:s * L + m] = R.clamp_ref(x[s * seg:s * seg + m])
    return Case("k_clamp_ms", f"T{T}-spf{spf}-tv{'.'.join(map(str, tv))}", qtts.CO_CLAMP_MS,
                [x, np.array(tv, np.int32)], [y0], (L, spf, n), (seg,), model=model,
                check=lambda outs: float(not same(outs[0], want) and _fail("clamp_ms: a sample behind the valid ones")),
                muts=("all",), meta=dict(x=x, L=L))


def clamp_twin_case(T, spf):
    c = clamp_ms_case(T, spf, (T,))
    L = c.meta["L"]
    v = c.meta["x"][:L]
    c.twin = Case("k_clamp", "twin", qtts.CO_CLAMP, [], [with_tail(v)], (L,),
                  model=lambda outs, mut: outs[0].__setitem__(slice(0, L), R.clamp_ref(outs[0][:L])),
                  check=lambda outs: 0.0)
    c.twin_same = lambda mine, other: same(mine[0], other[0])
    c.name = "twin-" + c.name
    return c


def copy2d_case(rows, cols, ldd, lds):
    rng = _rng("copy2d", rows, cols)
    src = np.full(rows * lds, NANF, np.float32)
    sidx = np.arange(rows)[:, None] * lds + np.arange(cols)[None, :]
    didx = np.arange(rows)[:, None] * ldd + np.arange(cols)[None, :]
    src[sidx] = rng.standard_normal((rows, cols)).astype(np.float32)
    d0 = sent(rows * ldd + TAIL)
    want = d0.copy()
    want[didx] = src[sidx]

    def model(outs, mut):
        outs[0][didx] = src[sidx]
    return Case("k_copy2d", f"{rows}x{cols}-ldd{ldd}-lds{lds}", qtts.CO_COPY2D, [src], [d0], (ldd, lds, rows, cols),
                model=model, check=lambda outs: float(not same(outs[0], want) and _fail("copy2d")))


# ------------------------------------------------------------------ history
def hist_cases(C, H, mul, T=4, sid=(4, 0, 2), tv=(4, 1, 3), ns=5):
    """the pair of launches around a conv: out 0 (slot -> margin), then out 1
    (the last H valid columns of [margin | new] -> slot) on what out 0 left"""
    n, L = len(sid), T * mul
    ldx = LM + L + RM
    seg = C * ldx + 17
    rng = _rng("hist", C, H, mul, T, sid, tv)
    hist0 = with_tail(rng.standard_normal((ns, C, H)).astype(np.float32))
    x0 = np.full(n * seg + TAIL, NANF, np.float32)
    for s in range(n):
        x0[s * seg:s * seg + C * ldx].reshape(C, ldx)[:, LM:LM + L] = rng.standard_normal((C, L))
    ints = [np.array(sid, np.int32), np.array(tv, np.int32)]
    name = f"C{C}-H{H}-mul{mul}-tv{'.'.join(map(str, tv))}"

    def run_in(hist, x, mut=()):
        for s in range(n):
            slot = s if "sid" in mut else sid[s]
            for c in range(C):
                base = s * seg + c * ldx + LM
                x[base - H:base] = hist[(slot * C + c) * H:(slot * C + c + 1) * H]

    def run_out(hist, x, mut=()):
        for s in range(n):
            slot = s if "sid" in mut else sid[s]
            end = L if "from_L" in mut else tv[s] * mul
            for c in range(C):
                base = s * seg + c * ldx + LM
                hist[(slot * C + c) * H:(slot * C + c + 1) * H] = x[base + end - H:base + end]
    x1 = x0.copy()
    run_in(hist0, x1)
    hist1 = hist0.copy()
    run_out(hist1, x1)
    # by the definition: the history is the last H columns of [old history | the valid new columns]
    for s in range(n):
        for c in range(C):
            old = hist0[(sid[s] * C + c) * H:(sid[s] * C + c + 1) * H]
            new = x0[s * seg + c * ldx + LM:][:tv[s] * mul]
            assert same(np.concatenate([old, new])[-H:], hist1[(sid[s] * C + c) * H:(sid[s] * C + c + 1) * H])
    assert np.all(np.isfinite(hist1[:-TAIL]))

    def checker(want_h, want_x):
        def check(outs):
            assert same(outs[0], want_h), "the slots: a stream's slot is wrong or another slot was written"
            assert same(outs[1], want_x), "the planes"
            return 0.0
        return check
    a = Case("k_hist_ms", name + "-in", qtts.CO_HIST_MS, ints, [hist0, (x0, LM)], (ldx, C, H, mul, n, 0), (seg,),
             model=lambda outs, mut: run_in(outs[0], outs[1], mut), check=checker(hist0, x1), muts=("sid",))
    b = Case("k_hist_ms", name + "-out", qtts.CO_HIST_MS, ints, [hist0, (x1, LM)], (ldx, C, H, mul, n, 1), (seg,),
             model=lambda outs, mut: run_out(outs[0], outs[1], mut), check=checker(hist1, x1), muts=("sid", "from_L"),
             meta=dict(C=C, H=H, L=L, ldx=ldx))
    return [a, b]


def hist_twin_case(C, H, mul, T=4):
    """n = 1, sid (0), tv = T: the save equals the single stream's copy2d"""
    b = hist_cases(C, H, mul, T, (0,), (T,), 1)[1]
    m = b.meta
    x1 = b.out[1][0]
    b.twin = Case("k_copy2d", "twin", qtts.CO_COPY2D, [(x1, LM + m["L"] - H)], [b.out[0]], (H, m["ldx"], C, H),
                  model=lambda outs, mut: None, check=lambda outs: 0.0)
    b.twin.model = lambda outs, mut: outs[0].__setitem__(slice(None), b.run_model()[0])
    b.twin_same = lambda mine, other: same(mine[0], other[0])
    b.name = "twin-" + b.name
    return b


# ------------------------------------------------------------------ keep-shift
def kv_shift_case(kvd, keepmax=72, S=80, T=8, nl2=4, ns=6):
    """streams: below the window; exactly at it; one row over (shift 1); well
    over (shift tv); hl + T crosses but hl + tv does not (must not move)"""
    sid, hl, tv = (5, 0, 3, 1, 4), (10, 64, 65, 72, 66), (8, 8, 8, 8, 3)
    n = len(sid)
    assert [h + t - keepmax for h, t in zip(hl, tv)] == [-54, 0, 1, 8, -3] and hl[4] + T > keepmax
    kv0 = with_tail(np.arange(nl2 * ns * S * kvd, dtype=np.float32))     # every element its own (layer, stream, row, column) code
    assert kv0[-TAIL - 1] < 2 ** 24

    def run(kv, mut=()):
        for s in range(n):
            tot = hl[s] + (T if "hl_T" in mut else tv[s])
            keep = min(tot, keepmax)
            shift = tot - keep
            if shift == 0:
                continue
            shift += ("plus" in mut) - ("minus" in mut)
            for l2 in range(nl2):
                p = ((l2 * ns + sid[s]) * S) * kvd
                for i in range(keep):                          # the upward walk, as in place as the kernel's
                    if shift:
                        kv[p + i * kvd:p + (i + 1) * kvd] = kv[p + (i + shift) * kvd:p + (i + shift + 1) * kvd]
    want = kv0.copy()
    promised = np.ones(kv0.shape, bool)         # rows >= keep of a shifted stream are left as they were: not asserted
    for s in range(n):
        tot = hl[s] + tv[s]
        shift = max(0, tot - keepmax)
        for l2 in range(nl2):
            p = ((l2 * ns + sid[s]) * S) * kvd
            if shift:
                want[p:p + keepmax * kvd] = kv0[p + shift * kvd:p + (shift + keepmax) * kvd]
                promised[p + keepmax * kvd:p + S * kvd] = False

    def check(outs):
        assert same(outs[0][promised], want[promised]), np.argwhere(outs[0][promised] != want[promised])[:4]
        return 0.0
    ints = [np.array(a, np.int32) for a in (sid, hl, tv)]
    return Case("k_kv_shift_ms", f"kvd{kvd}", qtts.CO_KV_SHIFT_MS, ints, [kv0], (ns, S, kvd, keepmax, n, nl2),
                model=lambda outs, mut: run(outs[0], mut), check=check, muts=("plus", "minus", "hl_T"))


# ------------------------------------------------------------------ snapshots and reset
def state_cases(kvn, elems=(8, 9, 11), ns=3, stride=32):
    """nh = 3 history parts of 4k, 4k + 1, 4k + 3 floats (the second on a base
    that is 4-byte aligned only: the scalar path), two K/V planes of `stride`
    floats a stream with kvn valid ones.  save stream 1, then load into stream 2
    of a differently filled state; then reset stream 0"""
    nh, nkv = len(elems), 2
    kvpad = (kvn + 3) // 4 * 4
    soff, pos = [], 0
    for e in elems:
        soff.append(pos)
        pos += (e + 3) // 4 * 4
    soff.append(pos)
    snap_n = pos + nkv * kvpad
    el = list(elems) + [stride] * nkv
    offs = [0, 1, 0, 0, 0]                       # part 1 starts one float into its buffer

    def state(seed):
        rng = _rng("state", seed, kvn)
        return [np.concatenate([sent(offs[y]), with_tail(rng.standard_normal(ns * el[y]).astype(np.float32))])
                for y in range(nh + nkv)]
    A, B = state(0), state(1)
    snap0 = sent(snap_n + TAIL)
    ptrs = ("ptrs", [(y, offs[y]) for y in range(nh + nkv)])
    tabs = [np.array(el, np.int32), np.array(soff, np.int32)]
    most = max(elems)

    def part(y):
        return (soff[y] if y < nh else soff[nh] + (y - nh) * kvpad), (el[y] if y < nh else kvn)

    def save(outs, mut=(), stream=1):            # outs: the nh + nkv state buffers, then the snapshot
        for y in range(nh + nkv):
            o, cnt = part(y)
            outs[-1][o:o + cnt] = outs[y][offs[y] + stream * el[y]:][:cnt]

    def load(outs, snap, stream=2):
        for y in range(nh + nkv):
            o, cnt = part(y)
            outs[y][offs[y] + stream * el[y]:][:cnt] = snap[o:o + cnt]
    after_save = [a.copy() for a in A] + [snap0.copy()]
    save(after_save)
    snap1 = after_save[-1]
    after_load = [b.copy() for b in B]
    load(after_load, snap1)
    for y in range(nh + nkv):                    # the definition: stream 2 of B now holds stream 1 of A, nothing else moved
        cnt = part(y)[1]
        assert same(after_load[y][offs[y] + 2 * el[y]:][:cnt], A[y][offs[y] + el[y]:][:cnt])
        rest = np.ones(B[y].shape, bool)
        rest[offs[y] + 2 * el[y]:offs[y] + 2 * el[y] + cnt] = False
        assert same(after_load[y][rest], B[y][rest])
    after_reset = [a.copy() for a in A[:nh]]
    for y in range(nh):
        after_reset[y][offs[y]:offs[y] + el[y]] = 0

    def eq(want):
        def check(outs):
            for y, w in enumerate(want):
                assert same(outs[y], w), ("buffer", y)
            return 0.0
        return check
    nn = (nh, nkv, most, 0, kvn, kvpad)
    sv = Case("k_ms_state_save", f"kvn{kvn}", qtts.CO_MS_STATE_SAVE, [ptrs] + tabs, [snap0] + A,
              nn[:3] + (1,) + nn[4:], model=lambda outs, mut: save(outs[1:] + outs[:1]),
              check=eq([snap1] + A))
    sv.inp[0] = ("ptrs", [(y + 1, offs[y]) for y in range(nh + nkv)])
    ld = Case("k_ms_state_load", f"kvn{kvn}", qtts.CO_MS_STATE_LOAD, [ptrs] + tabs + [snap1], B,
              nn[:3] + (2,) + nn[4:], model=lambda outs, mut: load(outs, snap1), check=eq(after_load))

    def reset(outs, mut):
        for y in range(nh):
            outs[y][offs[y]:offs[y] + el[y]] = 0
    rs = Case("k_hist_reset_ms", f"kvn{kvn}", qtts.CO_HIST_RESET_MS, [("ptrs", [(y, offs[y]) for y in range(nh)]),
                                                                     np.array(el[:nh], np.int32)],
              A[:nh], (nh, most, 0), model=reset, check=eq(after_reset))
    for c, k in ((sv, 1), (ld, 0), (rs, 0)):
        c.meta["nout"] = k                        # the other buffers are reached through the pointer table, not out[]
    return [sv, ld, rs]


# ------------------------------------------------------------------ the table
def build():
    cs = []
    cs += [rvq_sum_case(32, 16, 3), rvq_sum_case(40, 16, 67), rvq_sum_case(256, 16, 3), rvq_sum_case(40, 1, 1)]
    cs += [rvq_sum_case(40, 16, 4, ms=(2, (4, 1, 3))), rvq_sum_case(256, 16, 3, ms=(0, (3, 2))),
           rvq_sum_case(32, 1, 1, ms=(3, (1,)))]
    cs += [rvq_proj_case(32, 64, 3), rvq_proj_case(40, 10, 67), rvq_proj_case(256, 512, 3), rvq_proj_case(40, 7, 1)]
    cs += [rvq_proj_case(40, 10, 3, n=3), rvq_proj_case(256, 64, 1, n=2)]
    cs += [dwconv_case(5, 67, 7, False, True), dwconv_case(5, 67, 7, True, True), dwconv_case(300, 3, 7, True, False),
           dwconv_case(3, 1, 7, True, True), dwconv_case(4, 67, 1, False, True), dwconv_case(1024, 3, 7, False, False)]
    cs += [dwconv_case(5, 67, 7, True, True, n=3), dwconv_case(300, 3, 7, False, False, n=2)]
    cs += [ln_t_case(C, L) for C, L in ((128, 3), (300, 67), (1024, 7), (300, 1))]
    cs += [ln_t_case(300, 7, n=3), ln_t_case(1024, 1, n=2)]
    cs += [rms_rows_case(M, D) for M, D in ((3, 128), (67, 300), (7, 1024), (1, 300))]
    cs += [rope_rows_case(4, 16, 3), rope_rows_case(16, 64, 67), rope_rows_case(5, 64, 1)]
    kv = dict(sid=(4, 0, 2), pos0=(3, 0, 150), hl=(3, 0, 70), tv=(4, 1, 3), ns=5, S=80)
    cs += [rope_kv_case(4, 4, 16, 4, **kv), rope_kv_case(16, 5, 64, 4, **kv), rope_kv_case(16, 16, 64, 4, **kv)]
    cs += [ms_index_case((0,), (0,), 1), ms_index_case((4, 0, 2), (3, 0, 70), 5),
           ms_index_case((4, 0, 2, 1, 3), (1, 2, 3, 4, 5), 67)]
    cs += [clamp_case(300), clamp_case(1), clamp_ms_case(4, 75, (4, 1, 3)), clamp_ms_case(1, 3, (1,))]
    cs += [copy2d_case(5, 67, 70, 80), copy2d_case(1, 1, 1, 1), copy2d_case(67, 5, 5, 9)]
    for C, H, mul in ((300, 1, 1), (50, 6, 2), (5, 54, 8), (50, 6, 8)):
        cs += hist_cases(C, H, mul)
    cs += [kv_shift_case(64), kv_shift_case(320), kv_shift_case(1024)]
    cs += state_cases(0) + state_cases(10)
    return cs


def build_twins():
    """n = 1, sid (0) launches of the multi-stream kernels with the single-plane
    launch each must equal bit for bit"""
    tw = []
    a, b = rvq_sum_case(40, 16, 5, ms=(0, (5,)), seed=3), None
    cb = a.inp[2]
    rows = R.rvq_rows(a.inp[0], [0], 18, 0, 5, (5,))[:, :16]
    b = Case("k_rvq_sum", "twin", qtts.CO_RVQ_SUM, [np.ascontiguousarray(rows).reshape(-1), cb],
             [o.copy() for o in a.out], (5, 16, 12, 40), model=a.model, check=lambda outs: 0.0)
    a.twin, a.twin_same = b, lambda mine, other: same(mine[0], other[0]) and same(mine[1], other[1])
    a.name = "twin-" + a.name
    tw.append(a)
    for ms, one in ((rvq_proj_case(40, 10, 5, n=1), rvq_proj_case(40, 10, 5)),
                    (dwconv_case(5, 67, 7, True, True, n=1), dwconv_case(5, 67, 7, True, True)),
                    (ln_t_case(300, 7, n=1), ln_t_case(300, 7))):
        # the same generator key but n: give the twin the multi-stream case's operands
        one.inp = ms.inp
        one.model, one.check = ms.model, (lambda outs: 0.0)
        ms.twin, ms.twin_same = one, (lambda mine, other: same(mine[0], other[0]))
        ms.name = "twin-" + ms.name
        tw.append(ms)
    tw += [rope_twin_case(16, 5, 64, 3), clamp_twin_case(4, 75), hist_twin_case(50, 6, 2)]
    return tw


CASES = build()
TWINS = build_twins()
KERNELS = ["k_rvq_sum", "k_rvq_proj", "k_rvq_sum_ms", "k_rvq_proj_ms", "k_dwconv", "k_dwconv_ms", "k_ln_t", "k_ln_t_ms",
           "k_rms_rows", "k_rope_rows", "k_rope_kv_ms", "k_ms_index", "k_clamp", "k_copy2d", "k_clamp_ms", "k_hist_ms",
           "k_kv_shift_ms", "k_hist_reset_ms", "k_ms_state_save", "k_ms_state_load"]
