// qtts_runtime.hip - device model, weight layout in HBM, generation state and
// the qtts_dev_* C-ABI of include/qtts_hip.h but its codec entries
// (qtts_rt_codec.hip); the launches of a frame and its graphs are in
// qtts_rt_frame.hip, the kernel-level hooks in qtts_rt_hooks.hip, the context
// they share in qtts_dev.h.
//
// HBM layout (per device, one model, B slots):
//   talker layer l:  wqkv [(NH+2KV)*HD, H] bf16   fused q|k|v rows
//                    wo   [H, NH*HD]            bf16
//                    wgu  [2I, H]               bf16   gate/up interleaved in row quads
//                                                      (g0..g3 u0..u3 g4..g7 u4..u7 ...)
//                    wdown[H, I]                bf16
//                    q/k norm [HD], in/post norm [H] f32
//   sub-talker: same per layer; codec embeddings [G-1][Vs][H] and lm heads
//               [G-1][Vs][Hs] contiguous so a pass selects its table by offset
//   KV caches fp32 (as the reference, T.c:191-196): talker [L][B][S][KV*HD],
//               sub-talker [Ls][B][G][KVs*HDs]
//   codec: f32 tensors by name (k_codec.hip)
//
// One frame (group-0 sample + 15 sub-talker groups + next embedding) is ONE
// captured HIP graph; position / row / stop state lives in device memory so
// the same graph replays every frame with no host round trip.
#include "qtts_dev.h"

namespace {

float host_bf16(uint16_t v) {
    uint32_t u = (uint32_t)v << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint16_t host_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + (((u >> 16) & 1) + 0x7FFF)) >> 16);
}
float host_f16(uint16_t h) {
    _Float16 x;
    memcpy(&x, &h, 2);
    return (float)x;
}

}  // namespace

// ----------------------------------------------------------------- helpers
static constexpr size_t QTTS_ARENA_SMALL = (size_t)1 << 20, QTTS_ARENA_BLOCK = (size_t)32 << 20;
void *dalloc(qtts_dev *dv, size_t n, bool weight) {
    void *p = nullptr;
    if (n == 0) n = 16;
    // (off by default: +1.2 % in one same-box A/B, -1.3 % in the next,
    // profiles/r04g_ab_arena.txt; read per call: tests switch it per model)
    const char *ae = getenv("QTTS_HIP_ARENA");
    const int arena = ae ? atoi(ae) : 0;
    if (arena && n <= QTTS_ARENA_SMALL) {
        unsigned char *&base = weight ? dv->war : dv->sar;
        size_t &off = weight ? dv->war_off : dv->sar_off, &cap = weight ? dv->war_cap : dv->sar_cap;
        const size_t need = (n + 255) & ~(size_t)255;
        if (!base || off + need > cap) {
            void *blk = dalloc(dv, QTTS_ARENA_BLOCK, weight);   // (recorded in wallocs / sallocs)
            if (!blk) return nullptr;
            base = (unsigned char *)blk; off = 0; cap = QTTS_ARENA_BLOCK;
        }
        p = base + off;
        off += need;
        return p;
    }
    const hipError_t prior = hipPeekAtLastError();
    const hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
        fprintf(stderr, "qtts: hipMalloc(%zu) failed: %s (last error before it: %s)\n", n, hipGetErrorName(e),
                hipGetErrorName(prior));
        return nullptr;
    }
    if (weight) { dv->wallocs.push_back(p); dv->wbytes += n; }
    else { dv->sallocs.push_back(p); dv->sbytes += n; }
    return p;
}

void drop_row_graphs(qtts_dev *dv) {
    for (auto &g : dv->gNr)
        if (g) { hipGraphExecDestroy(g); g = nullptr; }
}

// drops forcing and taps with their buffers (the frame graphs that hold the
// pointers become invalid with them)
static void free_force(qtts_dev *dv) {
    if (!dv->f_armed) return;
    hipStreamSynchronize(dv->st);
    for (void *p : {(void *)dv->f_forced, (void *)dv->f_drawn, (void *)dv->f_taps, (void *)dv->f_tap_meta,
                    (void *)dv->f_tap_logits})
        if (p) hipFree(p);
    dv->f_forced = dv->f_drawn = dv->f_taps = dv->f_tap_meta = nullptr;
    dv->f_tap_logits = nullptr;
    dv->f_tap_ld = dv->f_ntaps = 0;
    dv->sbytes -= dv->f_bytes;
    dv->f_bytes = 0;
    dv->f_armed = false;
    dv->graph_key = -1;
}

// drops the per-slot parameter table (the frame graphs that hold its pointer
// become invalid with it)
static void free_slot_params(qtts_dev *dv) {
    if (!dv->sp_armed) return;
    hipStreamSynchronize(dv->st);
    if (dv->sp_tab) {
        hipFree(dv->sp_tab);
        dv->sbytes -= dv->sp_host.size() * sizeof(SampSlotRow);
    }
    dv->sp_tab = nullptr;
    dv->sp_host.clear();
    dv->sp_armed = dv->sp_general = false;
    dv->graph_key = -1;
}

static void free_state(qtts_dev *dv) {
    free_force(dv);
    free_slot_params(dv);
    dv->f_phase = 0;
    if (dv->g0) { hipGraphExecDestroy(dv->g0); dv->g0 = nullptr; }
    if (dv->gN) { hipGraphExecDestroy(dv->gN); dv->gN = nullptr; }
    drop_row_graphs(dv);
    for (void *p : dv->sallocs) hipFree(p);
    dv->sallocs.clear();
    dv->sbytes = 0;
    dv->sar = nullptr; dv->sar_off = dv->sar_cap = 0;
    dv->nb = 0;
    dv->nrun = 0;
    dv->ids_cap = 0;  // prompt scratch lived in sallocs
    dv->pids = dv->pplan = nullptr;
    dv->pt1 = dv->pproj = nullptr;
    dv->fed = false;
    dv->tf_open = dv->tf_gate = dv->tf_held = nullptr;
    dv->tf_eos = dv->tf_xsave = dv->tf_t1 = nullptr;
    dv->graph_key = -1;
    codec_free_state(&dv->codec);
}

static std::vector<float> to_f32(const void *host, int dtype, size_t n) {
    std::vector<float> o(n);
    if (dtype == 0) memcpy(o.data(), host, n * 4);
    else if (dtype == 1) for (size_t i = 0; i < n; ++i) o[i] = host_bf16(((const uint16_t *)host)[i]);
    else for (size_t i = 0; i < n; ++i) o[i] = host_f16(((const uint16_t *)host)[i]);
    return o;
}

static float *upload_f32(qtts_dev *dv, const void *host, int dtype, size_t n) {
    std::vector<float> f = to_f32(host, dtype, n);
    float *p = (float *)dalloc(dv, n * 4, true);
    if (!p || hipMemcpy(p, f.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}

static int upload_bf16_at(bf16_t *dst, const void *host, int dtype, size_t n) {
    if (dtype == 1) return hipMemcpy(dst, host, n * 2, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    std::vector<uint16_t> t(n);
    std::vector<float> f = to_f32(host, dtype, n);
    for (size_t i = 0; i < n; ++i) t[i] = host_to_bf16(f[i]);
    return hipMemcpy(dst, t.data(), n * 2, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

static bf16_t *upload_bf16(qtts_dev *dv, const void *host, int dtype, size_t n) {
    bf16_t *p = (bf16_t *)dalloc(dv, n * 2, true);
    if (!p || upload_bf16_at(p, host, dtype, n)) return nullptr;
    return p;
}

// ----------------------------------------------------------------- weights
static int put_layer(qtts_dev *dv, Layer &ly, const std::string &suf, const void *host, int dtype, size_t n,
                     int H, int NH, int KV, int HD, int I) {
    const size_t qd = (size_t)NH * HD, kd = (size_t)KV * HD;
    const size_t qkv_rows = qd + 2 * kd;
    if (suf == "self_attn.q_proj.weight" || suf == "self_attn.k_proj.weight" || suf == "self_attn.v_proj.weight") {
        if (!ly.wqkv) ly.wqkv = (bf16_t *)dalloc(dv, qkv_rows * H * 2, true);
        if (!ly.wqkv) return -1;
        size_t off = suf[10] == 'q' ? 0 : suf[10] == 'k' ? qd : qd + kd;
        size_t rows = suf[10] == 'q' ? qd : kd;
        if (n != rows * H) { fprintf(stderr, "qtts: %s has %zu elements, expected %zu\n", suf.c_str(), n, rows * H); return -1; }
        return upload_bf16_at(ly.wqkv + off * H, host, dtype, n);
    }
    if (suf == "self_attn.o_proj.weight") {
        if (n != (size_t)H * qd) return -1;
        ly.wo = upload_bf16(dv, host, dtype, n);
        return ly.wo ? 0 : -1;
    }
    if (suf == "mlp.gate_proj.weight" || suf == "mlp.up_proj.weight") {
        if (n != (size_t)I * H || I % 4) return -1;
        if (!ly.wgu) ly.wgu = (bf16_t *)dalloc(dv, (size_t)2 * I * H * 2, true);
        if (!ly.wgu) return -1;
        const bool up = suf[4] == 'u';
        std::vector<uint16_t> tmp;
        const void *src = host;
        if (dtype != 1) {
            tmp.resize(n);
            std::vector<float> f = to_f32(host, dtype, n);
            for (size_t i = 0; i < n; ++i) tmp[i] = host_to_bf16(f[i]);
            src = tmp.data();
        }
        // quad q of gate -> rows 8q..8q+3, of up -> rows 8q+4..8q+7
        const size_t quad = (size_t)4 * H * 2;
        return hipMemcpy2D((char *)ly.wgu + (up ? quad : 0), 2 * quad, src, quad, quad, I / 4,
                           hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    }
    if (suf == "mlp.down_proj.weight") {
        if (n != (size_t)H * I) return -1;
        ly.wdown = upload_bf16(dv, host, dtype, n);
        return ly.wdown ? 0 : -1;
    }
    float **f = suf == "self_attn.q_norm.weight" ? &ly.qn : suf == "self_attn.k_norm.weight" ? &ly.kn
              : suf == "input_layernorm.weight" ? &ly.in : suf == "post_attention_layernorm.weight" ? &ly.post : nullptr;
    if (f) {
        *f = upload_f32(dv, host, dtype, n);
        return *f ? 0 : -1;
    }
    return 0;  // unused tensor
}

static int parse_idx(const std::string &name, const std::string &pre, std::string *rest) {
    if (name.compare(0, pre.size(), pre) != 0) return -1;
    size_t p = pre.size(), q = p;
    while (q < name.size() && isdigit((unsigned char)name[q])) ++q;
    if (q == p || q >= name.size() || name[q] != '.') return -1;
    *rest = name.substr(q + 1);
    return atoi(name.c_str() + p);
}

extern "C" int qtts_dev_put_tensor(qtts_dev_t *dv, const char *cname, const void *host, int dtype,
                                   const int64_t *shape, int ndim) {
    if (!dv || !cname || !host) return -1;
    hipSetDevice(dv->device);
    std::string name(cname), rest;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    const qtts_dims_t &d = dv->d;
    int rc = 0, idx;
    const int er = enc_put_tensor(&dv->enc, name, host, dtype, shape, ndim, n);
    if (er < 0) { fprintf(stderr, "qtts: failed to take encoder tensor %s\n", cname); return -1; }
    if (er > 0) return 0;
    if (name.compare(0, 8, "decoder.") == 0) {
        rc = codec_put_tensor(&dv->codec, name, host, dtype, shape, ndim, n);
    } else if (name == "talker.model.codec_embedding.weight") {
        dv->codec_emb = upload_bf16(dv, host, dtype, n); rc = dv->codec_emb ? 0 : -1;
    } else if (name == "talker.model.text_embedding.weight") {
        dv->text_emb = upload_bf16(dv, host, dtype, n); rc = dv->text_emb ? 0 : -1;
    } else if (name == "talker.text_projection.linear_fc1.weight") {
        dv->fc1w = upload_bf16(dv, host, dtype, n); rc = dv->fc1w ? 0 : -1;
    } else if (name == "talker.text_projection.linear_fc1.bias") {
        dv->fc1b = upload_f32(dv, host, dtype, n); rc = dv->fc1b ? 0 : -1;
    } else if (name == "talker.text_projection.linear_fc2.weight") {
        dv->fc2w = upload_bf16(dv, host, dtype, n); rc = dv->fc2w ? 0 : -1;
    } else if (name == "talker.text_projection.linear_fc2.bias") {
        dv->fc2b = upload_f32(dv, host, dtype, n); rc = dv->fc2b ? 0 : -1;
    } else if (name == "talker.model.norm.weight") {
        dv->tk_norm = upload_f32(dv, host, dtype, n); rc = dv->tk_norm ? 0 : -1;
    } else if (name == "talker.codec_head.weight") {
        dv->head = upload_bf16(dv, host, dtype, n); rc = dv->head ? 0 : -1;
    } else if (name == "talker.code_predictor.small_to_mtp_projection.weight") {
        dv->st_proj = upload_bf16(dv, host, dtype, n); rc = dv->st_proj ? 0 : -1;
    } else if (name == "talker.code_predictor.small_to_mtp_projection.bias") {
        dv->st_projb = upload_f32(dv, host, dtype, n); rc = dv->st_projb ? 0 : -1;
    } else if (name == "talker.code_predictor.model.norm.weight") {
        dv->st_norm = upload_f32(dv, host, dtype, n); rc = dv->st_norm ? 0 : -1;
    } else if ((idx = parse_idx(name, "talker.code_predictor.model.codec_embedding.", &rest)) >= 0 && rest == "weight") {
        if (idx >= d.G - 1 || n != (size_t)d.Vs * d.H) { fprintf(stderr, "qtts: bad %s\n", cname); return -1; }
        if (!dv->st_emb) dv->st_emb = (bf16_t *)dalloc(dv, (size_t)(d.G - 1) * d.Vs * d.H * 2, true);
        rc = dv->st_emb ? upload_bf16_at(dv->st_emb + (size_t)idx * d.Vs * d.H, host, dtype, n) : -1;
    } else if ((idx = parse_idx(name, "talker.code_predictor.lm_head.", &rest)) >= 0 && rest == "weight") {
        if (idx >= d.G - 1 || n != (size_t)d.Vs * d.Hs) { fprintf(stderr, "qtts: bad %s\n", cname); return -1; }
        if (!dv->lm) dv->lm = (bf16_t *)dalloc(dv, (size_t)(d.G - 1) * d.Vs * d.Hs * 2, true);
        rc = dv->lm ? upload_bf16_at(dv->lm + (size_t)idx * d.Vs * d.Hs, host, dtype, n) : -1;
    } else if ((idx = parse_idx(name, "talker.code_predictor.model.layers.", &rest)) >= 0) {
        if (idx >= d.Ls) return 0;
        rc = put_layer(dv, dv->sl[idx], rest, host, dtype, n, d.Hs, d.NHs, d.KVs, d.HDs, d.Is);
    } else if ((idx = parse_idx(name, "talker.model.layers.", &rest)) >= 0) {
        if (idx >= d.L) return 0;
        rc = put_layer(dv, dv->tl[idx], rest, host, dtype, n, d.H, d.NH, d.KV, d.HD, d.I);
    } else {
        return 0;
    }
    if (rc) {
        fprintf(stderr, "qtts: failed to upload tensor %s\n", cname);
        return -1;
    }
    dv->got.insert(name);
    return 0;
}

extern "C" qtts_dev_t *qtts_dev_create(const qtts_dims_t *dims, int device) {
    if (hipSetDevice(device) != hipSuccess) {
        fprintf(stderr, "qtts: cannot select HIP device %d\n", device);
        return nullptr;
    }
    qtts_dev *dv = new qtts_dev();
    dv->d = *dims;
    dv->device = device;
    if (hipStreamCreateWithFlags(&dv->st, hipStreamNonBlocking) != hipSuccess) {
        delete dv;
        return nullptr;
    }
    dv->tl.resize(dims->L);
    dv->sl.resize(dims->Ls);
    // debug switches: QTTS_HIP_BSPLIT=0 batch O / down
    // projections without split-K; QTTS_HIP_ATTN_O=0 sub-talker attention and
    // O projection as two kernels
    const char *bs = getenv("QTTS_HIP_BSPLIT");
    dv->bsplit = !(bs && !atoi(bs));
    const char *bk = getenv("QTTS_HIP_BKZ_MAX");
    if (bk) dv->bkz_max = atoi(bk) < 1 ? 1 : atoi(bk) > 4 ? 4 : atoi(bk);
    const char *bw = getenv("QTTS_HIP_BKZ_WIDE");
    dv->bkz_wide = bw ? atoi(bw) : 1;
    const char *bm = getenv("QTTS_HIP_BSELF_MIN");
    if (bm) dv->bself_min = atoi(bm);
    const char *ad = getenv("QTTS_HIP_ATTN_DEFER");
    dv->attn_defer = !(ad && !atoi(ad));
    const char *lk = getenv("QTTS_HIP_ATTN_LPK");
    dv->attn_lpk = lk ? atoi(lk) : 0;
    const char *ao = getenv("QTTS_HIP_ATTN_O");
    dv->attn_o = !(ao && !atoi(ao));
    const char *pg = getenv("QTTS_HIP_PGEMM");
    dv->pgemm = !(pg && !atoi(pg));
    // QTTS_HIP_KV=bf16|fp32: the talker KV cache's element type (default fp32)
    const char *kvd = getenv("QTTS_HIP_KV");
    if (kvd && *kvd) {
        if (!strcmp(kvd, "bf16")) dv->kv_want = 1;
        else if (strcmp(kvd, "fp32")) fprintf(stderr, "qtts: QTTS_HIP_KV=%s ignored (bf16 or fp32)\n", kvd);
    }
    // QTTS_HIP_PREFIX_CACHE=<entries>: the instruct prefix cache's capacity (default 16, 0 off)
    const char *pc = getenv("QTTS_HIP_PREFIX_CACHE");
    if (pc && *pc) dv->pfx_cap = atoi(pc) < 0 ? 0 : atoi(pc);
    const char *tb = getenv("QTTS_HIP_TAB0B");
    dv->tab0b = !(tb && !atoi(tb));
    const char *sp = getenv("QTTS_HIP_ST_PAIR");
    dv->st_pair = !(sp && !atoi(sp));
    const char *pf = getenv("QTTS_HIP_L2PF");
    if (pf) dv->l2pf = atoi(pf);
    const char *pft = getenv("QTTS_HIP_L2PF_TK");
    if (pft) dv->l2pf_tk = atoi(pft);
    const char *gd = getenv("QTTS_HIP_GM_DBG");
    if (gd) dv->gm_dbg_layer = atoi(gd);
    codec_init(&dv->codec, dims, dv->st);
    dv->enc.st = dv->st;
    dv->enc.device = device;
    return dv;
}

// drops the least recently used prefix entries until at most `keep` are left
// (the stream is drained first: a queued save or restore may still use one)
static void prefix_evict(qtts_dev *dv, size_t keep) {
    if (dv->pfx.size() <= keep) return;
    hipStreamSynchronize(dv->st);
    while (dv->pfx.size() > keep) {
        size_t lru = 0;
        for (size_t i = 1; i < dv->pfx.size(); ++i)
            if (dv->pfx[i].used < dv->pfx[lru].used) lru = i;
        hipFree(dv->pfx[lru].buf);
        dv->pfx.erase(dv->pfx.begin() + lru);
    }
}

extern "C" int qtts_dev_prefix_cache(qtts_dev_t *dv, int max_entries) {
    if (!dv || max_entries < 0) return -1;
    hipSetDevice(dv->device);
    dv->pfx_cap = max_entries;
    prefix_evict(dv, (size_t)max_entries);
    return 0;
}

extern "C" size_t qtts_dev_prefix_cache_bytes(const qtts_dev_t *dv) {
    size_t n = 0;
    if (dv)
        for (const auto &e : dv->pfx) n += e.bytes;
    return n;
}

static std::atomic<long long> g_prefix_hits{0}, g_prefix_misses{0};
extern "C" long long qtts_hip_prefix_hits(void) { return g_prefix_hits.load(); }
extern "C" long long qtts_hip_prefix_misses(void) { return g_prefix_misses.load(); }

extern "C" void qtts_dev_destroy(qtts_dev_t *dv) {
    if (!dv) return;
    hipSetDevice(dv->device);
    hipStreamSynchronize(dv->st);
    prefix_evict(dv, 0);
    free_state(dv);
    snapshots_orphan(dv);
    codec_destroy(&dv->codec);
    enc_destroy(&dv->enc);
    if (dv->cst) hipStreamSynchronize(dv->cst);
    if (dv->hstop) hipHostFree(dv->hstop);
    for (hipEvent_t e : dv->fev)
        if (e) hipEventDestroy(e);
    for (CodecModel *ln : dv->clanes) codec_lane_delete(ln);
    for (hipStream_t st : dv->clane_st) hipStreamDestroy(st);
    if (dv->mwav) hipFree(dv->mwav);
    if (dv->mcodes) hipFree(dv->mcodes);
    if (dv->cwav) hipFree(dv->cwav);
    if (dv->pwav) hipFree(dv->pwav);
    if (dv->push_codes) hipFree(dv->push_codes);
    if (dv->cev) hipEventDestroy(dv->cev);
    if (dv->cst) hipStreamDestroy(dv->cst);
    for (void *p : dv->wallocs) hipFree(p);
    hipStreamDestroy(dv->st);
    delete dv;
}

extern "C" size_t qtts_dev_bytes(const qtts_dev_t *dv, int which) {
    if (!dv) return 0;
    return which == 0 ? dv->wbytes + codec_weight_bytes(&dv->codec) + enc_weight_bytes(&dv->enc) : dv->sbytes;
}

extern "C" int qtts_dev_set_kv_dtype(qtts_dev_t *dv, int dtype) {
    if (!dv || (dtype != 0 && dtype != 1)) return -1;
    dv->kv_want = dtype;   // (the state changes at the next qtts_dev_begin)
    return 0;
}

extern "C" int qtts_dev_kv_dtype(const qtts_dev_t *dv) { return dv ? dv->kv_want : -1; }

extern "C" int qtts_dev_get_kv(qtts_dev_t *dv, int layer, int b, int pos0, int n, float *k_host, float *v_host) {
    if (!dv || !dv->kc || !dv->vc || dv->nb < 1 || layer < 0 || layer >= dv->d.L || b < 0 || b >= dv->nb ||
        pos0 < 0 || n < 1 || pos0 > dv->S - n)
        return -1;
    hipSetDevice(dv->device);
    const size_t KVD = (size_t)dv->d.KV * dv->d.HD, cnt = (size_t)n * KVD, esz = dv->kv_esz();
    const size_t off = ((size_t)b * dv->S + pos0) * KVD * esz;
    CK(hipStreamSynchronize(dv->st));
    float *caches[2] = {dv->kc, dv->vc}, *outs[2] = {k_host, v_host};
    std::vector<uint16_t> tmp(dv->kv_dtype == 1 ? cnt : 0);
    for (int i = 0; i < 2; ++i) {
        if (!outs[i]) continue;
        const char *src = reinterpret_cast<const char *>(dv->kv_layer(caches[i], layer)) + off;
        if (dv->kv_dtype == 1) {
            CK(hipMemcpy(tmp.data(), src, cnt * 2, hipMemcpyDeviceToHost));
            for (size_t j = 0; j < cnt; ++j) outs[i][j] = host_bf16(tmp[j]);
        } else {
            CK(hipMemcpy(outs[i], src, cnt * 4, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

extern "C" int qtts_dev_get_hidden(qtts_dev_t *dv, int b, float *host) {
    if (!dv || !dv->x_tk || !host || b < 0 || b >= dv->nb) return -1;
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    CK(hipMemcpy(host, dv->x_tk + (size_t)b * dv->d.H, (size_t)dv->d.H * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int qtts_dev_get_attn(qtts_dev_t *dv, float *qkv_host, float *att_host) {
    if (!dv || dv->nb < 1 || !dv->qkv || !dv->att) return -1;
    if (att_host && !dv->att_own) {
        fprintf(stderr, "qtts_dev_get_attn: the last talker pass left no merged attention output "
                        "(batch 1 defers the merge to the O projection; QTTS_HIP_ATTN_DEFER=0 keeps it)\n");
        return -1;
    }
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    if (qkv_host) CK(hipMemcpy(qkv_host, dv->qkv, (size_t)dv->nb * dv->QKV() * 4, hipMemcpyDeviceToHost));
    if (att_host) CK(hipMemcpy(att_host, dv->att, (size_t)dv->nb * dv->d.NH * dv->d.HD * 4, hipMemcpyDeviceToHost));
    return 0;
}

// RoPE tables with the reference's exact libm arithmetic (T.c:97-113)
static int build_rope(qtts_dev *dv, int npos, int hd, float theta, float **cs, float **sn) {
    std::vector<float> c((size_t)npos * hd), s((size_t)npos * hd);
    const int half = hd / 2;
    for (int p = 0; p < npos; ++p)
        for (int i = 0; i < half; ++i) {
            float freq = 1.0f / powf(theta, (float)(2 * i) / (float)hd);
            float ang = (float)p * freq;
            c[(size_t)p * hd + i] = c[(size_t)p * hd + i + half] = cosf(ang);
            s[(size_t)p * hd + i] = s[(size_t)p * hd + i + half] = sinf(ang);
        }
    *cs = (float *)dalloc(dv, c.size() * 4, true);
    *sn = (float *)dalloc(dv, s.size() * 4, true);
    if (!*cs || !*sn) return -1;
    CK(hipMemcpy(*cs, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(*sn, s.data(), s.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int qtts_dev_finalize(qtts_dev_t *dv) {
    const qtts_dims_t &d = dv->d;
    hipSetDevice(dv->device);
    auto need = [&](const std::string &n) {
        if (!dv->got.count(n)) { fprintf(stderr, "Error: missing required tensor: %s\n", n.c_str()); return false; }
        return true;
    };
    bool ok = need("talker.model.codec_embedding.weight") && need("talker.model.text_embedding.weight") &&
              need("talker.text_projection.linear_fc1.weight") && need("talker.text_projection.linear_fc2.weight") &&
              need("talker.model.norm.weight") && need("talker.codec_head.weight") &&
              need("talker.code_predictor.model.norm.weight");
    static const char *lsuf[] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                                 "self_attn.o_proj.weight", "self_attn.q_norm.weight", "self_attn.k_norm.weight",
                                 "input_layernorm.weight", "post_attention_layernorm.weight", "mlp.gate_proj.weight",
                                 "mlp.up_proj.weight", "mlp.down_proj.weight"};
    for (int l = 0; ok && l < d.L; ++l)
        for (const char *s : lsuf) ok = ok && need("talker.model.layers." + std::to_string(l) + "." + s);
    for (int l = 0; ok && l < d.Ls; ++l)
        for (const char *s : lsuf) ok = ok && need("talker.code_predictor.model.layers." + std::to_string(l) + "." + s);
    for (int g = 0; ok && g < d.G - 1; ++g) {
        ok = ok && need("talker.code_predictor.model.codec_embedding." + std::to_string(g) + ".weight");
        ok = ok && need("talker.code_predictor.lm_head." + std::to_string(g) + ".weight");
    }
    if (ok && d.H != d.Hs) ok = need("talker.code_predictor.small_to_mtp_projection.weight");
    if (!ok) return -1;
    // (head sizes: what qtts_attention serves -- its generic kernel is wrong
    // for a head size that is no power of two)
    if (!qtts_attn_head_ok(d.HD) || !qtts_attn_head_ok(d.HDs) || d.G > 32) {
        fprintf(stderr, "Error: unsupported head_dim (talker=%d subtalker=%d) or code groups %d\n", d.HD, d.HDs, d.G);
        return -1;
    }
    // every decode GEMV's reduction width (qtts_gemv streams 64-column blocks)
    const int widths[] = {d.H, d.I, d.NH * d.HD, d.Hs, d.Is, d.NHs * d.HDs, d.TH};
    for (int c : widths)
        if (c % 64) {
            fprintf(stderr, "Error: unsupported layer width %d (hidden / intermediate / heads x head_dim must be "
                            "multiples of 64)\n", c);
            return -1;
        }
    if (d.V > 4096 || d.Vs > 4096) {
        fprintf(stderr, "Error: vocab > 4096 unsupported by the device sampler\n");
        return -1;
    }
    const char *pt = getenv("QTTS_HIP_PTAB");
    const bool ptab_on = !(pt && !atoi(pt));
    if (dv->st_proj && ptab_on) CKI(build_proj_tables(dv));
    if (ptab_on) CKI(build_qkv0_table(dv));
    CKI(codec_finalize(&dv->codec));
    // the streaming codec's state for up to 4096 frames, allocated now so the
    // first streaming request of a process does not pay for it (its buffers
    // are reused by every later stream of <= 4096 frames; longer ones re-grow)
    if (codec_stream_begin(&dv->codec, 4096) != 0)
        fprintf(stderr, "qtts: streaming codec state not pre-allocated (allocated on first use)\n");
    return enc_finalize(&dv->enc, d.H);
}

// ----------------------------------------------------------------- voice-clone encoders
extern "C" int qtts_dev_enc_config(qtts_dev_t *dv, const qtts_enc_dims_t *dims) {
    if (!dv || !dims) return -1;
    return enc_set_dims(&dv->enc, dims);
}

extern "C" int qtts_dev_enc_available(qtts_dev_t *dv) {
    if (!dv) return 0;
    return (dv->enc.spk_ready ? 1 : 0) | (dv->enc.mimi_ready ? 2 : 0);
}

extern "C" int qtts_dev_speaker_embed(qtts_dev_t *dv, int nb, const float *const *wav, const int *n, float *out,
                                      float *mel_out) {
    if (!dv || !wav || !n || !out) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    return enc_speaker(&dv->enc, nb, wav, n, out, mel_out);
}

extern "C" int qtts_dev_encode_audio(qtts_dev_t *dv, int nb, const float *const *wav, const int *n, int *codes,
                                     int max_frames, int *frames, float *latent) {
    if (!dv || !wav || !n || !codes || !frames) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    return enc_codes(&dv->enc, nb, wav, n, codes, max_frames, frames, latent);
}

// ----------------------------------------------------------------- state
static int alloc_state(qtts_dev *dv, int nb, int max_frames, int max_prefill) {
    const qtts_dims_t &d = dv->d;
    free_state(dv);
    if (dv->kv_dtype != dv->kv_want) prefix_evict(dv, 0);   // (entries hold the other element type)
    dv->kv_dtype = dv->kv_want;
    dv->nb = nb;
    dv->nrun = nb;
    dv->max_frames = max_frames;
    dv->p_cap = max_prefill;
    dv->S = max_prefill + max_frames + 1;
    dv->tr_cap = 4096;  // trailing rows per slot (text length bound)
    dv->rows_cap = nb * max_prefill;
    const size_t B = nb;
#define A(ptr, type, cnt)                                                 \
    do {                                                                  \
        dv->ptr = (type *)dalloc(dv, (size_t)(cnt) * sizeof(type), false); \
        if (!dv->ptr) return -1;                                          \
    } while (0)
    A(x_tk, float, B * d.H);
    A(qkv, float, B * dv->QKV());
    A(att, float, B * d.NH * d.HD);
    A(hbuf, float, B * d.I);
    A(logits, float, B * d.V);
    A(tk_hid, float, B * d.H);
    // (two rows at one slot: the batch-1 sub-talker runs positions 0 and 1 as a pair)
    const size_t B2 = B < 2 ? 2 : B;
    A(x_st, float, B2 * d.Hs);
    A(x_st2, float, B2 * d.Hs);
    A(x_tk2, float, B * d.H);
    A(bpo, float, (size_t)4 * B * (d.H > d.Hs ? d.H : d.Hs));
    A(bpd, float, (size_t)4 * B * (d.H > d.Hs ? d.H : d.Hs));
    A(ppart, float, (size_t)4 * 16 * (d.H > d.Hs ? d.H : d.Hs));
    A(opart, float, (size_t)B2 * ((size_t)d.KVs * d.Hs > (size_t)d.KV * d.H ? (size_t)d.KVs * d.Hs : (size_t)d.KV * d.H));
    A(qkv_s, float, B2 * dv->QKVs());
    A(att_s, float, B * d.NHs * d.HDs);
    A(h_s, float, B2 * d.Is);
    A(logits_s, float, B * d.Vs);
    {   // (bf16: half the elements' worth of floats; L B S KV HD is even -- HD is a multiple of 8)
        const size_t kv_floats = (size_t)d.L * B * dv->S * d.KV * d.HD * dv->kv_esz() / 4;
        A(kc, float, kv_floats);
        A(vc, float, kv_floats);
    }
    A(kcs, float, (size_t)d.Ls * B * d.G * d.KVs * d.HDs);
    A(vcs, float, (size_t)d.Ls * B * d.G * d.KVs * d.HDs);
    A(codes, int, B * (max_frames + 1) * d.G);
    A(counts, int, B * d.V);
    A(n_gen, int, B);
    A(stopped, int, B);
    A(cur_row, int, B);
    A(last_tok, int, B);
    CK(hipMemsetAsync(dv->last_tok, 0, B * sizeof(int), dv->st));
    A(stop_step, int, B);
    A(kv_len, int, B);
    A(n_trailing, int, B);
    A(rng, uint32_t, B);
    A(st_rng, uint32_t, B);
    A(trailing, float, B * 64 * d.H);  // grown on demand in qtts_dev_prompt
    dv->tr_cap = 64;
    A(prefill, float, B * max_prefill * d.H);
    A(pad_emb, float, d.H);
    const size_t R = dv->rows_cap;
    A(px, float, R * d.H);
    A(pqkv, float, R * dv->QKV());
    A(patt, float, R * d.NH * d.HD);
    A(ph, float, R * d.I);
    A(prow_b, int, R);
    A(ppos, int, R);
    A(psrc, int, R);
    A(plast, int, B);
    dv->pinv_cap = dv->rows_cap > 64 ? dv->rows_cap : 64;
    A(pinv, float, dv->pinv_cap);
    {
        // the prefill GEMM's split-K partials, sized by the rule its split
        // follows (qtts_mgemm_part_elems: 4 M floats = 16 MB at the defaults, fewer
        // for short prompts); QTTS_HIP_MGEMM_KZ=0: no scratch, no split
        const size_t wide = std::max<size_t>({(size_t)dv->QKV(), (size_t)2 * d.I, (size_t)d.H, (size_t)d.TH});
        const char *e = getenv("QTTS_HIP_MGEMM_KZ");
        dv->mpart_elems = e && !strcmp(e, "0") ? 0 : qtts_mgemm_part_elems(std::max<size_t>(R, 64), wide);
        // (k_pgemm splits K while its 128 x 128 tiles x columns stay under 512:
        // at most 512 x 128 x 128 partials, 8 columns of every row)
        if (dv->mpart_elems)
            dv->mpart_elems = std::max(dv->mpart_elems, std::min<size_t>((size_t)512 * 128 * 128, (size_t)8 * R * wide));
        if (dv->mpart_elems) A(mpart, float, dv->mpart_elems);
        const size_t kmax = std::max<size_t>({(size_t)d.H, (size_t)d.I, (size_t)d.NH * d.HD});
        dv->pplanes_elems = dv->pgemm ? qtts_pgemm_plane_elems(R, kmax) : 0;
        if (dv->pplanes_elems) A(pplanes, unsigned short, dv->pplanes_elems);
    }
    {
        const int gph = d.NH / d.KV;
        // partial slots for the smaller split size of the two launch forms
        const int ch = std::min(qtts_attn_keys_per_split(d.HD, false, dv->attn_lpk),
                                qtts_attn_keys_per_split(d.HD, true, dv->attn_lpk));
        dv->att_nsplit = (dv->S + ch - 1) / ch;
        A(att_part, float, B * d.KV * dv->att_nsplit * (gph * d.HD + 2 * gph));
        const int kvmax = d.KV > d.KVs ? d.KV : d.KVs;
        A(att_cnt, int, B * kvmax);
        CK(hipMemsetAsync(dv->att_cnt, 0, B * kvmax * sizeof(int), dv->st));
        A(pf_sink, unsigned, 1);
        A(btick, int, QTTS_GM_TICKS);
        CK(hipMemsetAsync(dv->btick, 0, QTTS_GM_TICKS * sizeof(int), dv->st));
        if (dv->gm_dbg_layer >= 0) {
            A(gm_dbg, unsigned long long, 4 * 2048 * 8);
            CK(hipMemsetAsync(dv->gm_dbg, 0, 4 * 2048 * 8 * 8, dv->st));
        }
    }
#undef A
    dv->p_len_h.assign(nb, 0);
    dv->n_tr_h.assign(nb, 0);
    dv->pfx_ids.assign(nb, std::vector<int>());
    CK(hipMemsetAsync(dv->codes, 0, B * (max_frames + 1) * d.G * sizeof(int), dv->st));
    CK(hipMemsetAsync(dv->kcs, 0, (size_t)d.Ls * B * d.G * d.KVs * d.HDs * 4, dv->st));
    CK(hipMemsetAsync(dv->vcs, 0, (size_t)d.Ls * B * d.G * d.KVs * d.HDs * 4, dv->st));
    // RoPE tables sized to the KV capacity
    if (dv->rope_max < dv->S) {
        dv->rope_max = dv->S;
        CKI(build_rope(dv, dv->S, d.HD, d.theta, &dv->rope_cos, &dv->rope_sin));
        if (d.HDs != d.HD) CKI(build_rope(dv, d.G + 2, d.HDs, d.theta, &dv->rope_cos_s, &dv->rope_sin_s));
        else { dv->rope_cos_s = dv->rope_cos; dv->rope_sin_s = dv->rope_sin; }
    }
    dv->graph_key = -1;
    return 0;
}

static int reset_counters(qtts_dev *dv) {
    const size_t B = dv->nb;
    hipStream_t st = dv->st;
    if (dv->hstop_cap < (int)B) {   // (a new pointer: the frame graphs are re-captured)
        if (dv->hstop) CK(hipHostFree(dv->hstop));
        dv->hstop = nullptr;
        CK(hipHostMalloc((void **)&dv->hstop, B * sizeof(int), hipHostMallocDefault));
        dv->hstop_cap = (int)B;
        dv->graph_key = -1;
    }
    if (!dv->fev[0]) {
        CK(hipEventCreateWithFlags(&dv->fev[0], hipEventDisableTiming));
        CK(hipEventCreateWithFlags(&dv->fev[1], hipEventDisableTiming));
    }
    CK(hipStreamSynchronize(st));   // no frame of a previous run still writes the mirror
    memset(dv->hstop, 0, B * sizeof(int));
    CK(hipMemsetAsync(dv->counts, 0, B * dv->d.V * sizeof(int), st));
    CK(hipMemsetAsync(dv->n_gen, 0, B * sizeof(int), st));
    CK(hipMemsetAsync(dv->stopped, 0, B * sizeof(int), st));
    CK(hipMemsetAsync(dv->cur_row, 0, B * sizeof(int), st));
    CK(hipMemsetAsync(dv->stop_step, 0, B * sizeof(int), st));
    std::vector<uint32_t> r(B, seed_bits(dv->par.seed));
    CK(hipMemcpyAsync(dv->rng, r.data(), B * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dv->st_rng, r.data(), B * 4, hipMemcpyHostToDevice, st));
    CK(hipStreamSynchronize(st));
    return 0;
}

// forcing is defined for one utterance per slot: the work queue's slot
// operations refuse while it is armed
static bool force_refuses(const qtts_dev *dv, const char *what) {
    if (!dv->f_armed) return false;
    fprintf(stderr, "qtts: %s refused: forced codes / taps are armed (not defined for the work queue)\n", what);
    return true;
}

// and so is incremental text input (qtts_dev_text_open)
static bool fed_refuses(const qtts_dev *dv, const char *what) {
    if (!dv->fed) return false;
    fprintf(stderr, "qtts: %s refused: the run takes its text incrementally (not defined for the work queue)\n", what);
    return true;
}

static bool same_params(const qtts_gen_params_t &a, const qtts_gen_params_t &b) {
    return memcmp(&a, &b, sizeof a) == 0;
}

// Above 16 slots every decode GEMV is one launch of the wide batch kernel
// (k_gemvx.hip) or nothing: a model with a weight shape it does not take is
// refused here, by name, instead of at the frame graph's capture.
static bool wide_shapes_ok(const qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    const struct { const char *name; int R, C; bool used; } sh[] = {
        {"talker q|k|v", dv->QKV(), d.H, true},
        {"talker O", d.H, d.NH * d.HD, true},
        {"talker gate|up", 2 * d.I, d.H, true},
        {"talker down", d.H, d.I, true},
        {"codec head", d.V, d.H, true},
        {"sub-talker input projection", d.Hs, d.H, dv->st_proj != nullptr},
        {"sub-talker q|k|v", dv->QKVs(), d.Hs, true},
        {"sub-talker O", d.Hs, d.NHs * d.HDs, true},
        {"sub-talker gate|up", 2 * d.Is, d.Hs, true},
        {"sub-talker down", d.Hs, d.Is, true},
        {"sub-talker lm head", d.Vs, d.Hs, true},
    };
    for (const auto &s : sh)
        if (s.used && !qtts_gemvx_shape_ok(s.R, s.C)) {
            fprintf(stderr, "qtts_dev_begin: more than 16 slots refused: the wide batch GEMV does not take the %s "
                            "weights [%d][%d] (rows %% 16, columns %% 32)\n", s.name, s.R, s.C);
            return false;
        }
    return true;
}

extern "C" int qtts_dev_begin(qtts_dev_t *dv, int nb, int max_frames, int max_prefill, const qtts_gen_params_t *p) {
    if (!dv || nb < 1 || max_frames < 1) return -1;
    if (nb > QTTS_HIP_MAX_BATCH) {
        fprintf(stderr, "qtts_dev_begin: %d slots refused (at most %d lock-step slots per context)\n", nb,
                QTTS_HIP_MAX_BATCH);
        return -1;
    }
    if (nb > 16 && !wide_shapes_ok(dv)) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));   // a prime left pending by a run that pushed no frames
    free_force(dv);        // forcing and taps last for one run (and their record until the next begins)
    free_slot_params(dv);  // and so do per-slot sampling parameters
    // and so does incremental text input (the fed frame graphs stay: graph_key tells the families
    // apart, so the next fed run on this state replays them and an unfed one captures the plain family)
    dv->fed = false;
    dv->f_run_frames = max_frames;
    if (max_prefill < 16) max_prefill = 16;
    // (another cache element type: new state, and with it new frame graphs)
    const bool realloc_ = nb != dv->nb || max_frames > dv->max_frames || max_prefill > dv->p_cap ||
                          dv->kv_want != dv->kv_dtype;
    if (realloc_) {
        if (dv->cst) CK(hipStreamSynchronize(dv->cst));   // a prime still reading the codec scratch
        dv->prime_pending = false;
        CKI(alloc_state(dv, nb, max_frames, max_prefill));
    }
    if (!dv->have_par || !same_params(dv->par, *p)) {
        dv->par = *p;
        dv->have_par = true;
        dv->graph_key = -1;
    }
    dv->nrun = dv->nb;
    CKI(reset_counters(dv));
    dv->f_phase = 1;
    return 0;
}

// ----------------------------------------------------------------- prompt + prefill
static int ensure_trailing(qtts_dev *dv, int n_tr) {
    if (n_tr <= dv->tr_cap) return 0;
    const qtts_dims_t &d = dv->d;
    int cap = dv->tr_cap;
    while (cap < n_tr) cap *= 2;
    float *nt = (float *)dalloc(dv, (size_t)dv->nb * cap * d.H * 4, false);
    if (!nt) return -1;
    CK(hipStreamSynchronize(dv->st));
    for (int b = 0; b < dv->nb; ++b)
        CK(hipMemcpy(nt + (size_t)b * cap * d.H, dv->trailing + (size_t)b * dv->tr_cap * d.H,
                     (size_t)dv->tr_cap * d.H * 4, hipMemcpyDeviceToDevice));
    dv->trailing = nt;  // old block stays in sallocs until free_state
    dv->tr_cap = cap;
    dv->graph_key = -1;
    return 0;
}

// voice-clone inputs for the next qtts_dev_prompt: reference codes
// [n_ref][G] (plan codec ids <= -3) and the speaker x-vector [H] (id -2)
extern "C" int qtts_dev_prompt_ref(qtts_dev_t *dv, const int *ref_codes, int n_ref, const float *spk) {
    if (!dv || n_ref < 0 || (n_ref > 0 && !ref_codes)) return -1;
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    if (!dv->pspk) {
        dv->pspk = (float *)dalloc(dv, (size_t)d.H * 4, true);
        if (!dv->pspk) return -1;
    }
    if (n_ref > dv->pref_cap) {
        const int cap = n_ref < 512 ? 512 : n_ref;
        dv->pref = (int *)dalloc(dv, (size_t)cap * d.G * 4, true);   // lives with the weights (freed at destroy)
        if (!dv->pref) return -1;
        dv->pref_cap = cap;
    }
    CK(hipStreamSynchronize(dv->st));
    if (n_ref > 0) CK(hipMemcpy(dv->pref, ref_codes, (size_t)n_ref * d.G * 4, hipMemcpyHostToDevice));
    if (spk) CK(hipMemcpy(dv->pspk, spk, (size_t)d.H * 4, hipMemcpyHostToDevice));
    dv->n_pref = n_ref;
    dv->has_spk = spk != nullptr;
    return 0;
}

extern "C" int qtts_dev_prompt(qtts_dev_t *dv, int b, const int *text_ids, int n_text, const int *plan, int nplan,
                               int p_len, int n_trailing, int pad_row) {
    if (!dv || b < 0 || b >= dv->nb || p_len > dv->p_cap || n_text < 1) return -1;
    // kind-2 rows (the cacheable prefix): the plan's leading rows, prompt rows
    // 0 .. n-1 of this slot in order, text alone (no codec id), and not the
    // whole prompt; assembled as kind 0
    std::vector<int> hplan, pids;
    for (int e = 0; e < nplan; ++e) {
        const int *r = plan + 5 * e;
        if (r[2] != 2) continue;
        if (hplan.empty()) hplan.assign(plan, plan + (size_t)5 * nplan);
        if (e != (int)pids.size() || r[4] != e || r[1] != -1 || r[3] != b || r[0] < 0 || r[0] >= n_text ||
            e + 1 >= p_len) {
            fprintf(stderr, "qtts_dev_prompt: plan row %d: prefix rows (kind 2) must be the leading rows 0..n-1 of "
                            "the slot's prompt, without a codec id, and fewer than p_len\n", e);
            return -1;
        }
        pids.push_back(text_ids[r[0]]);
        hplan[5 * e + 2] = 0;
    }
    if (!hplan.empty()) plan = hplan.data();
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    CKI(ensure_trailing(dv, n_trailing));
    CK(hipStreamSynchronize(dv->st));
    if (n_text > dv->ids_cap || nplan > 4 * dv->ids_cap) {
        int cap = n_text < 256 ? 256 : n_text;
        if (4 * cap < nplan) cap = (nplan + 3) / 4;
        dv->pids = (int *)dalloc(dv, (size_t)cap * 4, false);
        dv->pplan = (int *)dalloc(dv, (size_t)4 * cap * 5 * 4, false);   // 4 * cap plan rows of 5 ints
        dv->pt1 = (float *)dalloc(dv, (size_t)cap * d.TH * 4, false);
        dv->pproj = (float *)dalloc(dv, (size_t)cap * d.H * 4, false);
        if (!dv->pids || !dv->pplan || !dv->pt1 || !dv->pproj) return -1;
        dv->ids_cap = cap;
    }
    if (nplan > 4 * dv->ids_cap) return -1;
    CK(hipMemcpy(dv->pids, text_ids, (size_t)n_text * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv->pplan, plan, (size_t)nplan * 5 * 4, hipMemcpyHostToDevice));
    // text_embedding -> fc1 (+b, SiLU) -> fc2 (+b), 16 rows per launch (Q.c:823-847)
    {
        if (!dv->fc1b) { fprintf(stderr, "qtts: text projection without fc1 bias unsupported\n"); return -1; }
        GemvArgs a = gv(dv->fc1w, d.TH, d.TH, nullptr, 0, dv->pt1, d.TH, 1, EPI_BIAS_SILU);
        a.table = dv->text_emb; a.ids = dv->pids; a.ids_bstride = 1; a.bias = dv->fc1b;
        CKI(rows_proj(dv, a, n_text));
        a = gv(dv->fc2w, d.H, d.TH, dv->pt1, d.TH, dv->pproj, d.H, 1, dv->fc2b ? EPI_BIAS : EPI_STORE);
        a.bias = dv->fc2b;
        CKI(rows_proj(dv, a, n_text));
    }
    PromptArgs pa;
    pa.proj = dv->pproj; pa.plan = dv->pplan; pa.nplan = nplan; pa.H = d.H; pa.codec_emb = dv->codec_emb;
    pa.prefill = dv->prefill; pa.p_cap = dv->p_cap; pa.trailing = dv->trailing; pa.tr_cap = dv->tr_cap;
    pa.st_emb = dv->st_emb; pa.G = d.G; pa.V = d.V; pa.Vs = d.Vs;
    pa.spk = dv->has_spk ? dv->pspk : nullptr;
    pa.ref_codes = dv->n_pref > 0 ? dv->pref : nullptr; pa.n_ref = dv->n_pref;
    CKI(qtts_prompt_assemble(pa, dv->st));
    dv->n_pref = 0; dv->has_spk = 0;   // consumed
    if (pad_row >= 0) CK(hipMemcpyAsync(dv->pad_emb, dv->pproj + (size_t)pad_row * d.H, (size_t)d.H * 4,
                                        hipMemcpyDeviceToDevice, dv->st));
    CK(hipMemcpyAsync(dv->n_trailing + b, &n_trailing, 4, hipMemcpyHostToDevice, dv->st));
    CK(hipStreamSynchronize(dv->st));
    dv->p_len_h[b] = p_len;
    dv->n_tr_h[b] = n_trailing;
    dv->pfx_ids[b] = pids;
    return 0;
}

// one launch between slot b's cache rows [0, n) and a prefix entry
static int prefix_copy(qtts_dev *dv, const qtts_dev::PrefixEntry &e, int b, int save) {
    const size_t row = (size_t)dv->d.KV * dv->d.HD * dv->kv_esz(), n = e.ids.size();
    if (b < 0 || b >= dv->nb || (int)n > dv->S || e.dtype != dv->kv_dtype || e.bytes != 2 * dv->d.L * n * row) return -1;
    KvPrefixArgs a;
    a.kc = reinterpret_cast<char *>(dv->kc) + (size_t)b * dv->S * row;
    a.vc = reinterpret_cast<char *>(dv->vc) + (size_t)b * dv->S * row;
    a.entry = e.buf;
    a.layer_stride = (size_t)dv->nb * dv->S * row;
    a.chunk = n * row;
    a.L = dv->d.L; a.esz = (int)dv->kv_esz(); a.save = save;
    return qtts_kv_prefix_copy(a, dv->st);
}

// The prefix stages of a prefill of `slots` (qtts_dev_prefill / _refill).  A
// slot with a prefix always takes the same two passes, hit or miss, so its
// state never depends on what the cache holds:
//   1. once per distinct missing prefix: a prefill pass over its n rows alone,
//      into the first slot that needs it, and one save launch into a new entry;
//   2. every other slot with that prefix, and every hit: one restore launch.
// first[i] = the rows of slots[i] then in the cache (0: no prefix, or the cache
// is off and the prefix rows are ordinary rows of the one pass).  Save and
// restore are stream-ordered launches with no host wait; a miss waits once,
// for its own pass's row lists.
static int prefix_stages(qtts_dev *dv, const std::vector<int> &slots, std::vector<int> &first) {
    first.assign(slots.size(), 0);
    if (dv->pfx_cap < 1) return 0;
    for (size_t i = 0; i < slots.size(); ++i) {
        const int b = slots[i];
        const std::vector<int> &ids = dv->pfx_ids[b];
        if (ids.empty()) continue;
        const int n = (int)ids.size();
        qtts_dev::PrefixEntry *hit = nullptr;
        for (auto &e : dv->pfx)
            if (e.dtype == dv->kv_dtype && e.ids == ids) hit = &e;
        if (hit) {
            ++g_prefix_hits;
            hit->used = ++dv->pfx_clock;
            CKI(prefix_copy(dv, *hit, b, 0));
        } else {
            ++g_prefix_misses;
            std::vector<int> last;
            CKI(prefill_rows(dv, std::vector<int>{b}, std::vector<int>{n}, last));
            CK(hipStreamSynchronize(dv->st));   // (the pass's row lists are host vectors; a miss only)
            prefix_evict(dv, (size_t)dv->pfx_cap - 1);
            qtts_dev::PrefixEntry e;
            e.ids = ids; e.dtype = dv->kv_dtype; e.used = ++dv->pfx_clock;
            e.bytes = (size_t)2 * dv->d.L * n * dv->d.KV * dv->d.HD * dv->kv_esz();
            if (hipMalloc(&e.buf, e.bytes) != hipSuccess) {
                fprintf(stderr, "qtts: no memory for a prefix cache entry of %zu bytes\n", e.bytes);
                return -1;
            }
            dv->pfx.push_back(e);
            CKI(prefix_copy(dv, dv->pfx.back(), b, 1));
        }
        first[i] = n;
    }
    return 0;
}

// talker prefill over all slots' prompt rows (T.c:254-472)
extern "C" int qtts_dev_prefill(qtts_dev_t *dv) {
    if (!dv || dv->nb < 1) return -1;
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    hipStream_t st = dv->st;
    std::vector<int> slots(dv->nb), last, first;
    for (int b = 0; b < dv->nb; ++b) slots[b] = b;
    CKI(prefix_stages(dv, slots, first));
    CKI(prefill_rows(dv, slots, dv->p_len_h, last, &first));
    // last raw hidden of each slot -> x_tk; kv_len = prefill length
    CK(hipMemcpyAsync(dv->plast, last.data(), dv->nb * 4, hipMemcpyHostToDevice, st));
    CKI(qtts_copy_rows(dv->x_tk, d.H, dv->px, d.H, dv->plast, dv->nb, d.H, st));
    CK(hipMemcpyAsync(dv->kv_len, dv->p_len_h.data(), dv->nb * 4, hipMemcpyHostToDevice, st));
    CK(hipStreamSynchronize(st));
    return 0;
}

// Work queue: slot b of the live batch takes the utterance
// qtts_dev_prompt(b, ...) just assembled.  Its prompt rows but the last are
// prefilled (the KV cache positions 0 .. p_len - 2 of slot b); the last prompt
// row becomes the slot's talker input at kv_len = p_len - 1, so the next
// lock-step frame (the talker-first graph every running slot replays) runs
// that row through the talker at position p_len - 1 -- the same arithmetic the
// reference's prefill applies to it (T.c:254-472 vs T.c:478-533, the last
// row's hidden feeding codec_head, Q.c:1282-1295) -- then samples the
// utterance's frame 0.  The slot's counters start afresh (Q.c:1250-1270).
// Everything is ordered on the context stream after the frames already queued.
extern "C" int qtts_dev_refill(qtts_dev_t *dv, int b) {
    if (!dv || b < 0 || b >= dv->nb || dv->p_len_h[b] < 2) return -1;
    if (force_refuses(dv, "qtts_dev_refill") || fed_refuses(dv, "qtts_dev_refill")) return -1;
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    std::vector<int> last, first;
    CKI(prefix_stages(dv, std::vector<int>{b}, first));
    if (first[0] < dv->p_len_h[b] - 1)   // (a prompt of its prefix and one more row: nothing left for the pass)
        CKI(prefill_rows(dv, std::vector<int>{b}, std::vector<int>{dv->p_len_h[b] - 1}, last, &first));
    SlotResetArgs r;
    r.b = b; r.pos = dv->p_len_h[b] - 1; r.H = d.H; r.V = d.V;
    r.row = dv->prefill + ((size_t)b * dv->p_cap + r.pos) * d.H;
    r.x = dv->x_tk; r.kv_len = dv->kv_len; r.n_gen = dv->n_gen; r.cur_row = dv->cur_row; r.stopped = dv->stopped;
    r.stop_step = dv->stop_step; r.last_tok = dv->last_tok; r.counts = dv->counts;
    r.rng = dv->rng; r.st_rng = dv->st_rng;
    r.seed_bits = dv->sp_armed ? dv->sp_host[b].seed_bits : seed_bits(dv->par.seed);   // (the slot's own row)
    CKI(qtts_slot_reset(r, dv->st));
    CK(hipStreamSynchronize(dv->st));   // (the prefill's row lists are host vectors)
    // the host's stop mirror: no queued frame writes it for this slot (it was
    // stopped in all of them)
    if (dv->hstop && b < dv->hstop_cap) ((volatile int *)dv->hstop)[b] = 0;
    return 0;
}

// Work queue: stop slot b from the next queued frame on (its utterance reached
// max_new_tokens / the fixed length without EOS, Q.c:1282); stream-ordered.
extern "C" int qtts_dev_retire(qtts_dev_t *dv, int b) {
    if (!dv || b < 0 || b >= dv->nb) return -1;
    hipSetDevice(dv->device);
    CK(hipMemsetD32Async((hipDeviceptr_t)(dv->stopped + b), 1, 1, dv->st));
    return 0;
}

// ----------------------------------------------------------------- incremental text input
// frames a live slot was held for want of a text row, as the polls of fed runs
// saw them, since the library loaded
static std::atomic<long long> g_text_held{0};
extern "C" long long qtts_hip_text_held_frames(void) { return g_text_held.load(); }

// Slot b's text opens (after its qtts_dev_prompt, before frame 0).  The prompt
// carries the tts_eos row alone (n_trailing 1: a template with one content
// id); it moves to the slot's eos row, the count goes back to 0 and the run
// becomes a fed one.  Stream-ordered, no host wait.
extern "C" int qtts_dev_text_open(qtts_dev_t *dv, int b) {
    if (!dv || b < 0 || b >= dv->nb) return -1;
    if (dv->f_phase != 1) {
        fprintf(stderr, "qtts_dev_text_open: valid after qtts_dev_begin and before the first frame\n");
        return -1;
    }
    if (dv->f_armed) {
        fprintf(stderr, "qtts_dev_text_open refused: forced codes / taps are armed\n");
        return -1;
    }
    if (dv->n_tr_h[b] != 1) {
        fprintf(stderr, "qtts_dev_text_open: slot %d's prompt has %d trailing rows (the tts_eos row alone expected)\n",
                b, dv->n_tr_h[b]);
        return -1;
    }
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    const size_t B = dv->nb;
    if (!dv->tf_gate) {
        dv->tf_open = (int *)dalloc(dv, B * 4, false);
        dv->tf_gate = (int *)dalloc(dv, B * 4, false);
        dv->tf_held = (int *)dalloc(dv, B * 4, false);
        dv->tf_eos = (float *)dalloc(dv, B * d.H * 4, false);
        dv->tf_xsave = (float *)dalloc(dv, B * d.H * 4, false);
        dv->tf_t1 = (float *)dalloc(dv, (size_t)QTTS_TF_MAX * d.TH * 4, false);
        if (!dv->tf_open || !dv->tf_gate || !dv->tf_held || !dv->tf_eos || !dv->tf_xsave || !dv->tf_t1) {
            dv->tf_gate = nullptr;
            return -1;
        }
    }
    if (!dv->fed) {
        CK(hipMemsetAsync(dv->tf_open, 0, B * 4, dv->st));
        CK(hipMemsetAsync(dv->tf_gate, 0, B * 4, dv->st));
        CK(hipMemsetAsync(dv->tf_held, 0, B * 4, dv->st));
        dv->tf_rows.assign(B, 0);
        dv->tf_open_h.assign(B, 0);
        dv->tf_held_h.assign(B, 0);
        dv->fed = true;
    }
    CKI(qtts_text_open(dv->tf_eos + (size_t)b * d.H, dv->trailing + (size_t)b * dv->tr_cap * d.H, d.H, dv->n_trailing,
                       dv->tf_open, dv->tf_held, b, dv->st));
    dv->tf_rows[b] = 0;
    dv->tf_open_h[b] = 1;
    dv->n_tr_h[b] = 0;
    return 0;
}

extern "C" int qtts_dev_text_append(qtts_dev_t *dv, int b, const int *ids, int n, int close) {
    if (!dv || b < 0 || b >= dv->nb || n < 0 || (n > 0 && !ids) || (n == 0 && !close)) return -1;
    if (!dv->fed || !dv->tf_open_h[b]) {
        fprintf(stderr, "qtts_dev_text_append: slot %d's text is not open\n", b);
        return -1;
    }
    const qtts_dims_t &d = dv->d;
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= d.TV) {
            fprintf(stderr, "qtts_dev_text_append: text token id %d out of range\n", ids[i]);
            return -1;
        }
    hipSetDevice(dv->device);
    // (growth past tr_cap: the one append that waits, and the frame graphs are captured again)
    CKI(ensure_trailing(dv, dv->tf_rows[b] + n + (close ? 1 : 0)));
    TextFeedArgs a;
    a.b = b; a.text_emb = dv->text_emb; a.fc1w = dv->fc1w; a.fc2w = dv->fc2w; a.fc1b = dv->fc1b; a.fc2b = dv->fc2b;
    a.TH = d.TH; a.H = d.H; a.t1 = dv->tf_t1; a.trailing = dv->trailing; a.tr_cap = dv->tr_cap;
    a.n_trailing = dv->n_trailing; a.text_open = dv->tf_open; a.eos = dv->tf_eos + (size_t)b * d.H;
    if (!dv->fc1b) { fprintf(stderr, "qtts: text projection without fc1 bias unsupported\n"); return -1; }
    int i0 = 0;
    do {
        a.n = n - i0 < QTTS_TF_MAX ? n - i0 : QTTS_TF_MAX;
        for (int j = 0; j < a.n; ++j) a.ids[j] = ids[i0 + j];
        i0 += a.n;
        a.close = close && i0 == n;
        CKI(qtts_text_append(a, dv->st));
    } while (i0 < n);
    dv->tf_rows[b] += n + (close ? 1 : 0);
    if (close) dv->tf_open_h[b] = 0;
    dv->n_tr_h[b] = dv->tf_rows[b];
    return 0;
}

// measurement: the same append between two events on the context stream; waits for it
extern "C" int qtts_dev_text_append_ms(qtts_dev_t *dv, int b, const int *ids, int n, int close, float *ms) {
    if (!dv || !ms) return -1;
    hipSetDevice(dv->device);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0, dv->st));
    const int rc = qtts_dev_text_append(dv, b, ids, n, close);
    CK(hipEventRecord(e1, dv->st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return rc;
}

extern "C" int qtts_dev_get_trailing(qtts_dev_t *dv, int b, int row0, int n, float *host) {
    if (!dv || !host || b < 0 || b >= dv->nb || row0 < 0 || n < 1 || row0 + n > dv->tr_cap) return -1;
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    CK(hipMemcpy(host, dv->trailing + ((size_t)b * dv->tr_cap + row0) * dv->d.H, (size_t)n * dv->d.H * 4,
                 hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int qtts_dev_text_state(qtts_dev_t *dv, int b, int *rows, int *open, int *held) {
    if (!dv || b < 0 || b >= dv->nb) return -1;
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    if (rows) CK(hipMemcpy(rows, dv->n_trailing + b, 4, hipMemcpyDeviceToHost));
    if (open) { *open = 0; if (dv->tf_open) CK(hipMemcpy(open, dv->tf_open + b, 4, hipMemcpyDeviceToHost)); }
    if (held) { *held = 0; if (dv->tf_held) CK(hipMemcpy(held, dv->tf_held + b, 4, hipMemcpyDeviceToHost)); }
    return 0;
}

// Work queue, lagged as qtts_dev_frame_done: waits until frame `step` has
// finished and copies every slot's EOS mirror (1: drew EOS by then).
extern "C" int qtts_dev_frame_stops(qtts_dev_t *dv, int step, int *stopped) {
    if (!dv || !stopped || !dv->hstop) return -1;
    hipSetDevice(dv->device);
    if (dv->graph_key >= 1) CK(hipEventSynchronize(dv->fev[step & 1]));
    else CK(hipStreamSynchronize(dv->st));
    for (int b = 0; b < dv->nrun; ++b) stopped[b] = ((volatile int *)dv->hstop)[b] != 0;
    return 0;
}

// Work queue, tail of a run (no utterance left to admit): slot `from`'s
// whole decode state moves to slot `to` (a freed slot below it), so that the
// running slots are the first ones and qtts_dev_set_rows can launch fewer
// rows.  Stream-ordered; the caller has synchronised (no frame in flight
// writes either slot).
extern "C" int qtts_dev_move_slot(qtts_dev_t *dv, int from, int to) {
    if (!dv || from < 0 || to < 0 || from >= dv->nb || to >= dv->nb || from == to) return -1;
    if (force_refuses(dv, "qtts_dev_move_slot") || fed_refuses(dv, "qtts_dev_move_slot")) return -1;
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    hipStream_t st = dv->st;
    int kv = 0;
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(&kv, dv->kv_len + from, 4, hipMemcpyDeviceToHost));
    if (kv < 0 || kv >= dv->S) return -1;
    const size_t KVD = (size_t)d.KV * d.HD, esz = dv->kv_esz(), lstride = (size_t)dv->nb * dv->S * KVD * esz;
    const size_t w = (size_t)(kv + 1) * KVD * esz;   // positions 0 .. kv (the next step writes kv)
    for (float *c : {dv->kc, dv->vc})
        CK(hipMemcpy2DAsync((char *)c + (size_t)to * dv->S * KVD * esz, lstride,
                            (const char *)c + (size_t)from * dv->S * KVD * esz, lstride, w, d.L,
                            hipMemcpyDeviceToDevice, st));
    auto row = [&](void *base, size_t bytes) {
        return hipMemcpyAsync((char *)base + (size_t)to * bytes, (const char *)base + (size_t)from * bytes, bytes,
                              hipMemcpyDeviceToDevice, st);
    };
    CK(row(dv->x_tk, (size_t)d.H * 4));
    CK(row(dv->counts, (size_t)d.V * 4));
    CK(row(dv->codes, (size_t)(dv->max_frames + 1) * d.G * 4));
    CK(row(dv->trailing, (size_t)dv->tr_cap * d.H * 4));
    for (int *p : {dv->kv_len, dv->n_gen, dv->cur_row, dv->stopped, dv->stop_step, dv->last_tok, dv->n_trailing})
        CK(row(p, 4));
    CK(row(dv->rng, 4));
    CK(row(dv->st_rng, 4));
    if (dv->sp_armed) {   // the slot's sampling parameters travel with it
        CK(row(dv->sp_tab, sizeof(SampSlotRow)));
        dv->sp_host[to] = dv->sp_host[from];
    }
    CK(hipStreamSynchronize(st));
    dv->p_len_h[to] = dv->p_len_h[from];
    dv->n_tr_h[to] = dv->n_tr_h[from];
    dv->pfx_ids[to] = dv->pfx_ids[from];
    if (dv->hstop && from < dv->hstop_cap && to < dv->hstop_cap)
        ((volatile int *)dv->hstop)[to] = ((volatile int *)dv->hstop)[from];
    return 0;
}

// Work queue: the next frames launch the first `rows` slots only (1 <= rows
// <= the slots of qtts_dev_begin; their own graph per row count).
extern "C" int qtts_dev_set_rows(qtts_dev_t *dv, int rows) {
    if (!dv || rows < 1 || rows > dv->nb || (rows < dv->nb && rows > QTTS_MAX_SLOTS)) return -1;
    if (force_refuses(dv, "qtts_dev_set_rows") || (rows < dv->nb && fed_refuses(dv, "qtts_dev_set_rows"))) return -1;
    dv->nrun = rows;
    return 0;
}

// sizes the per-slot trailing text rows for the longest utterance a run will
// see (a later qtts_dev_prompt never grows them, so the frame graphs stay)
extern "C" int qtts_dev_reserve(qtts_dev_t *dv, int max_trailing) {
    if (!dv || max_trailing < 0) return -1;
    hipSetDevice(dv->device);
    return ensure_trailing(dv, max_trailing);
}

extern "C" int qtts_dev_frame(qtts_dev_t *dv, int step) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(ensure_graphs(dv));
    if (dv->nrun < dv->nb && step == 0) return -1;   // (frame 0 runs every slot)
    dv->f_phase = 2;
    if (dv->graph_key == 0) return record_frame(dv, step > 0);
    hipGraphExec_t g = step == 0 ? dv->g0 : dv->gN;
    if (dv->nrun < dv->nb) {
        hipGraphExec_t &gr = dv->gNr[dv->nrun];
        if (!gr) CKI(capture(dv, true, &gr));
        g = gr;
    }
    CK(hipGraphLaunch(g, dv->st));
    CK(hipEventRecord(dv->fev[step & 1], dv->st));
    return 0;
}

// EOS mode without a host round trip per frame: wait until frame `step` has
// finished (the caller has already queued frame step + 1) and report whether
// every running slot had drawn EOS by then.  At most one frame runs past the
// last stop, against up to poll_every - 1 with a synchronous poll (which also
// leaves the GPU idle until the next launch).
extern "C" int qtts_dev_frame_done(qtts_dev_t *dv, int step, int *all_stopped) {
    if (!dv || !all_stopped || !dv->hstop) return -1;
    hipSetDevice(dv->device);
    if (dv->graph_key >= 1) CK(hipEventSynchronize(dv->fev[step & 1]));
    else CK(hipStreamSynchronize(dv->st));
    int all = 1;
    for (int b = 0; b < dv->nrun; ++b) all &= ((volatile int *)dv->hstop)[b] != 0;
    *all_stopped = all;
    return 0;
}

extern "C" int qtts_dev_poll(qtts_dev_t *dv, int *stopped, int *n_gen, int *stop_step) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    const size_t B = dv->nb;
    if (stopped) CK(hipMemcpyAsync(stopped, dv->stopped, B * 4, hipMemcpyDeviceToHost, dv->st));
    if (n_gen) CK(hipMemcpyAsync(n_gen, dv->n_gen, B * 4, hipMemcpyDeviceToHost, dv->st));
    if (stop_step) CK(hipMemcpyAsync(stop_step, dv->stop_step, B * 4, hipMemcpyDeviceToHost, dv->st));
    std::vector<int> held;
    if (dv->fed) {   // the held counters ride along (qtts_hip_text_held_frames)
        held.resize(B);
        CK(hipMemcpyAsync(held.data(), dv->tf_held, B * 4, hipMemcpyDeviceToHost, dv->st));
    }
    CK(hipStreamSynchronize(dv->st));
    for (size_t b = 0; b < held.size(); ++b) {
        if (held[b] > dv->tf_held_h[b]) g_text_held.fetch_add(held[b] - dv->tf_held_h[b]);
        dv->tf_held_h[b] = held[b];
    }
    return 0;
}

extern "C" int qtts_dev_get_codes(qtts_dev_t *dv, int b, int *host_codes, int max_frames) {
    if (!dv || b < 0 || b >= dv->nb) return -1;
    hipSetDevice(dv->device);
    int n = 0;
    CK(hipMemcpyAsync(&n, dv->n_gen + b, 4, hipMemcpyDeviceToHost, dv->st));
    CK(hipStreamSynchronize(dv->st));
    if (dv->gm_dbg) {   // QTTS_HIP_GM_DBG: phase spans of the chosen talker layer's GEMVs, last frame
        std::vector<unsigned long long> h(4 * 2048 * 8);
        CK(hipMemcpy(h.data(), dv->gm_dbg, h.size() * 8, hipMemcpyDeviceToHost));
        static const char *op[4] = {"q|k|v", "O / -", "gate|up", "down"};
        // (k_gemvw: 3 epilogue, 4 after the prefetch sink, 5 weights issued,
        // 6 merged; k_gemvb: 2 = MFMAs done, 3 = after the final barrier,
        // 4 = after the epilogue stores, 5 = tiles summed, 6 = normalised)
        static const char *ph[7] = {"start", "x staged", "dot done", "epilogue", "pf landed", "w issued", "merged"};
        unsigned long long tq = 0;   // the first launch's first start: the launch offsets below
        for (int g = 0; g < 4; ++g) {
            const unsigned long long *b = h.data() + (size_t)g * 2048 * 8;
            unsigned long long t0 = ~0ull, tend = 0;
            for (int i = 0; i < 2048; ++i) if (b[i * 8] && b[i * 8] < t0) t0 = b[i * 8];
            for (int i = 0; i < 2048 * 8; ++i) if (b[i] > tend) tend = b[i];
            if (t0 != ~0ull) {
                if (!tq) tq = t0;
                fprintf(stderr, "[gm_dbg] %-8s launch at %7.2f us after the first, last stamp %6.2f us into it\n", op[g],
                        (t0 - tq) * 0.01, (tend - t0) * 0.01);
            }
            for (int k = 0; k < 7; ++k) {
                std::vector<double> v;
                for (int i = 0; i < 2048; ++i) if (b[i * 8 + k]) v.push_back((b[i * 8 + k] - t0) * 0.01);
                if (v.empty()) continue;
                std::sort(v.begin(), v.end());
                fprintf(stderr, "[gm_dbg] %-8s %-10s n %4zu  min %6.2f  med %6.2f  max %6.2f us\n", op[g], ph[k], v.size(),
                        v[0], v[v.size() / 2], v.back());
            }
        }
        hipMemsetAsync(dv->gm_dbg, 0, h.size() * 8, dv->st);
    }
    if (n > max_frames) n = max_frames;
    CK(hipMemcpyAsync(host_codes, dv->codes + (size_t)b * (dv->max_frames + 1) * dv->d.G, (size_t)n * dv->d.G * 4,
                      hipMemcpyDeviceToHost, dv->st));
    CK(hipStreamSynchronize(dv->st));
    return n;
}

// ----------------------------------------------------------------- teacher forcing, taps
// first arming after a qtts_dev_begin: the tables (everything free, nothing
// drawn, no tap) and the tap buffers; the frame graphs are captured anew
static int arm_force(qtts_dev *dv) {
    if (dv->f_phase != 1) {
        fprintf(stderr, "qtts: forced codes / taps are armed after qtts_dev_begin and before frame 0\n");
        return -1;
    }
    if (dv->f_armed) return 0;
    if (dv->sp_armed) {
        fprintf(stderr, "qtts: forced codes / taps refused: per-slot sampling parameters are armed for this run\n");
        return -1;
    }
    const qtts_dims_t &d = dv->d;
    const size_t tab = (size_t)dv->nb * (dv->max_frames + 1) * d.G * sizeof(int);
    const int ld = d.V > d.Vs ? d.V : d.Vs;
    const size_t taps = QTTS_MAX_TAPS * 3 * sizeof(int), meta = QTTS_MAX_TAPS * 4 * sizeof(int);
    const size_t lg = (size_t)QTTS_MAX_TAPS * ld * sizeof(float);
    dv->f_armed = true;   // (free_force releases whatever was allocated if one of these fails)
    CK(hipMalloc((void **)&dv->f_forced, tab));
    CK(hipMalloc((void **)&dv->f_drawn, tab));
    CK(hipMalloc((void **)&dv->f_taps, taps));
    CK(hipMalloc((void **)&dv->f_tap_meta, meta));
    CK(hipMalloc((void **)&dv->f_tap_logits, lg));
    dv->f_bytes = 2 * tab + taps + meta + lg;
    dv->sbytes += dv->f_bytes;
    dv->f_tap_ld = ld;
    dv->f_ntaps = 0;
    CK(hipMemsetAsync(dv->f_forced, 0xFF, tab, dv->st));
    CK(hipMemsetAsync(dv->f_drawn, 0xFF, tab, dv->st));
    CK(hipMemsetAsync(dv->f_taps, 0xFF, taps, dv->st));
    CK(hipMemsetAsync(dv->f_tap_meta, 0, meta, dv->st));
    CK(hipMemsetAsync(dv->f_tap_logits, 0, lg, dv->st));
    CK(hipStreamSynchronize(dv->st));
    dv->graph_key = -1;
    return 0;
}

extern "C" int qtts_dev_force(qtts_dev_t *dv, int b, const int *codes, int n_frames) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    const qtts_dims_t &d = dv->d;
    if (dv->f_phase != 1) return arm_force(dv);   // (refuses with its message)
    if (b < 0 || b >= dv->nb) {
        fprintf(stderr, "qtts_dev_force: slot %d out of range (%d slots)\n", b, dv->nb);
        return -1;
    }
    if (n_frames < 0 || n_frames > dv->f_run_frames || (n_frames > 0 && !codes)) {
        fprintf(stderr, "qtts_dev_force: %d frames outside [0, %d]\n", n_frames, dv->f_run_frames);
        return -1;
    }
    std::vector<int> h((size_t)n_frames * d.G);
    for (int f = 0; f < n_frames; ++f)
        for (int g = 0; g < d.G; ++g) {
            const int id = codes[(size_t)f * d.G + g];
            const bool ok = id < 0 || (g == 0 ? (id < d.V - 1024 || id == d.eos_id) && id < d.V : id < d.Vs);
            if (!ok) {
                fprintf(stderr, "qtts_dev_force: id %d at frame %d, group %d out of range\n", id, f, g);
                return -1;
            }
            h[(size_t)f * d.G + g] = id < 0 ? -1 : id;
        }
    CKI(arm_force(dv));
    // (a slot armed again: the later call replaces the earlier one)
    int *row = dv->f_forced + (size_t)b * (dv->max_frames + 1) * d.G;
    CK(hipMemset(row, 0xFF, (size_t)(dv->max_frames + 1) * d.G * sizeof(int)));
    if (n_frames > 0) CK(hipMemcpy(row, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int qtts_dev_tap(qtts_dev_t *dv, int b, int frame, int group) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    if (dv->f_phase != 1) return arm_force(dv);   // (refuses with its message)
    if (b < 0 || b >= dv->nb || frame < 0 || frame >= dv->f_run_frames || group < 0 || group >= dv->d.G) {
        fprintf(stderr, "qtts_dev_tap: (slot %d, frame %d, group %d) out of range\n", b, frame, group);
        return -1;
    }
    if (dv->f_armed && dv->f_ntaps >= QTTS_MAX_TAPS) {
        fprintf(stderr, "qtts_dev_tap: at most %d taps per run\n", QTTS_MAX_TAPS);
        return -1;
    }
    CKI(arm_force(dv));
    const int t[3] = {b, frame, group};
    CK(hipMemcpy(dv->f_taps + 3 * dv->f_ntaps, t, sizeof t, hipMemcpyHostToDevice));
    return dv->f_ntaps++;
}

extern "C" int qtts_dev_get_drawn(qtts_dev_t *dv, int b, int *host, int max_frames) {
    if (!dv || !dv->f_armed || b < 0 || b >= dv->nb || !host || max_frames < 0) return -1;
    hipSetDevice(dv->device);
    const int n = max_frames < dv->max_frames + 1 ? max_frames : dv->max_frames + 1;
    CK(hipStreamSynchronize(dv->st));
    if (n > 0)
        CK(hipMemcpy(host, dv->f_drawn + (size_t)b * (dv->max_frames + 1) * dv->d.G, (size_t)n * dv->d.G * sizeof(int),
                     hipMemcpyDeviceToHost));
    return n;
}

extern "C" int qtts_dev_get_tap(qtts_dev_t *dv, int i, float *logits_host, int max_n, unsigned *rng_bits, int *drawn) {
    if (!dv || !dv->f_armed || i < 0 || i >= dv->f_ntaps) return -1;
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    int m[4] = {0, 0, 0, 0};
    CK(hipMemcpy(m, dv->f_tap_meta + 4 * i, sizeof m, hipMemcpyDeviceToHost));
    if (!m[3]) return -1;   // the draw never happened (the slot had stopped, or the run ended before it)
    if (rng_bits) *rng_bits = (unsigned)m[1];
    if (drawn) *drawn = m[2];
    const int n = m[0] < max_n ? m[0] : max_n;
    if (logits_host && n > 0)
        CK(hipMemcpy(logits_host, dv->f_tap_logits + (size_t)i * dv->f_tap_ld, (size_t)n * sizeof(float),
                     hipMemcpyDeviceToHost));
    return m[0];
}

// ----------------------------------------------------------------- per-slot sampling parameters
static SampSlotRow slot_row_of(const qtts_slot_params_t &p) {
    SampSlotRow r;
    r.temp = p.temperature; r.top_p = p.top_p; r.rep = p.repetition_penalty; r.top_k = p.top_k;
    r.st_temp = p.st_temperature; r.st_top_p = p.st_top_p; r.st_top_k = p.st_top_k; r.seed_bits = seed_bits(p.seed);
    return r;
}

static bool slot_params_ok(const char *who, const qtts_slot_params_t &p) {
    const float f[5] = {p.temperature, p.top_p, p.repetition_penalty, p.st_temperature, p.st_top_p};
    for (float v : f)
        if (!std::isfinite(v)) {
            fprintf(stderr, "%s: a non-finite sampling parameter\n", who);
            return false;
        }
    if (p.top_p <= 0.0f || p.st_top_p <= 0.0f || p.repetition_penalty <= 0.0f) {
        fprintf(stderr, "%s: top_p %g / %g and repetition_penalty %g must be > 0\n", who, p.top_p, p.st_top_p,
                p.repetition_penalty);
        return false;
    }
    return true;
}

// both of the row's draws (talker over V ids, sub-talker over Vs) take the fast path
static bool slot_row_fast(const qtts_dev *dv, const SampSlotRow &r) {
    return qtts_sample_row_fast(r, 1, dv->d.V) && qtts_sample_row_fast(r, 0, dv->d.Vs);
}

extern "C" int qtts_dev_slot_params(qtts_dev_t *dv, int b, const qtts_slot_params_t *p) {
    if (!dv || !p) return -1;
    if (dv->f_phase < 1) {
        fprintf(stderr, "qtts_dev_slot_params: no run begun (call qtts_dev_begin first)\n");
        return -1;
    }
    if (b < 0 || b >= dv->nb) {
        fprintf(stderr, "qtts_dev_slot_params: slot %d out of range (%d slots)\n", b, dv->nb);
        return -1;
    }
    if (!slot_params_ok("qtts_dev_slot_params", *p)) return -1;
    if (dv->f_armed) {
        fprintf(stderr, "qtts_dev_slot_params: refused: forced codes / taps are armed for this run\n");
        return -1;
    }
    hipSetDevice(dv->device);
    if (!dv->sp_armed) {   // the first call of the run: every row from begin's parameters
        qtts_slot_params_t q;
        q.temperature = dv->par.temperature; q.top_p = dv->par.top_p; q.repetition_penalty = dv->par.repetition_penalty;
        q.top_k = dv->par.top_k; q.st_temperature = dv->par.st_temperature; q.st_top_p = dv->par.st_top_p;
        q.st_top_k = dv->par.st_top_k; q.seed = dv->par.seed;
        const SampSlotRow r0 = slot_row_of(q);
        std::vector<SampSlotRow> h((size_t)dv->nb, r0);
        SampSlotRow *t = nullptr;
        CK(hipMalloc((void **)&t, h.size() * sizeof(SampSlotRow)));
        if (hipMemcpy(t, h.data(), h.size() * sizeof(SampSlotRow), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(t);
            return -1;
        }
        // (the frames in flight, if any, hold the plain samplers: the new graphs are captured after them)
        dv->sp_tab = t;
        dv->sp_host.swap(h);
        dv->sbytes += dv->sp_host.size() * sizeof(SampSlotRow);
        dv->sp_armed = true;
        dv->sp_general = !slot_row_fast(dv, r0);
        dv->graph_key = -1;
    }
    const SampSlotRow r = slot_row_of(*p);
    if (!slot_row_fast(dv, r)) dv->sp_general = true;   // (ensure_graphs: the frames switch to the general kernel)
    const bool fresh = dv->f_phase == 1;   // before frame 0: the slot's RNG states start from this seed
    CKI(qtts_slot_row_set(dv->sp_tab, b, r, fresh ? dv->rng : nullptr, fresh ? dv->st_rng : nullptr, dv->st));
    dv->sp_host[b] = r;
    return 0;
}

extern "C" long long qtts_hip_sample_slot_launches(void) { return qtts_sample_slot_launches(); }

// ----------------------------------------------------------------- host-pointer stage wrappers
static int ensure_slot0(qtts_dev *dv) {
    if (dv->nb >= 1) return 0;
    qtts_gen_params_t p{0.9f, 1.0f, 1.05f, 50, 0.9f, 1.0f, 50, 0, 42};
    return qtts_dev_begin(dv, 1, 4096, 256, &p);
}

extern "C" int qtts_dev_talker_prefill_host(qtts_dev_t *dv, const float *embeds, int n, float *hidden_out) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(ensure_slot0(dv));
    if (n > dv->p_cap) {
        qtts_gen_params_t p = dv->par;
        CKI(qtts_dev_begin(dv, dv->nb, dv->max_frames > 4096 ? dv->max_frames : 4096, n, &p));
    } else if (dv->kv_want != dv->kv_dtype) {   // qtts_dev_set_kv_dtype since the state was allocated
        qtts_gen_params_t p = dv->par;
        CKI(qtts_dev_begin(dv, dv->nb, dv->max_frames, dv->p_cap, &p));
    }
    const qtts_dims_t &d = dv->d;
    for (int b = 0; b < dv->nb; ++b) {
        dv->p_len_h[b] = b == 0 ? n : 0;
        dv->pfx_ids[b].clear();
    }
    CK(hipMemcpy(dv->prefill, embeds, (size_t)n * d.H * 4, hipMemcpyHostToDevice));
    CKI(qtts_dev_prefill(dv));
    if (hidden_out) {
        dv->nrun = 1;   // slot 0's row of the prefill's hidden in x_tk, nothing pending
        dv->tk_res.reset(dv->x_tk, dv->x_tk2, d.H, 1);
        const GemvArgs a = talker_head_args(dv);
        dv->nrun = dv->nb;
        CKI(qtts_gemv(a, dv->st));
        CK(hipMemcpyAsync(hidden_out, dv->tk_hid, (size_t)d.H * 4, hipMemcpyDeviceToHost, dv->st));
        CK(hipStreamSynchronize(dv->st));
    }
    return 0;
}

extern "C" int qtts_dev_talker_forward_host(qtts_dev_t *dv, const float *embed, float *logits, float *hidden_out) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(ensure_slot0(dv));
    const qtts_dims_t &d = dv->d;
    dv->nrun = 1;  // slot 0 only
    int rc = 0;
    if (hipMemcpy(dv->x_tk, embed, (size_t)d.H * 4, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (!rc) rc = talker_layers(dv);
    if (!rc) rc = talker_tail(dv);
    dv->nrun = dv->nb;
    CKI(rc);
    int kl = 0;
    CK(hipMemcpyAsync(&kl, dv->kv_len, 4, hipMemcpyDeviceToHost, dv->st));
    CK(hipStreamSynchronize(dv->st));
    kl += 1;
    CK(hipMemcpy(dv->kv_len, &kl, 4, hipMemcpyHostToDevice));
    if (logits) CK(hipMemcpy(logits, dv->logits, (size_t)d.V * 4, hipMemcpyDeviceToHost));
    if (hidden_out) CK(hipMemcpy(hidden_out, dv->tk_hid, (size_t)d.H * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int qtts_dev_subtalker_host(qtts_dev_t *dv, const float *hidden, int first_code, int *out_codes) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(ensure_slot0(dv));
    const qtts_dims_t &d = dv->d;
    CK(hipStreamSynchronize(dv->st));
    CK(hipMemcpy(dv->tk_hid, hidden, (size_t)d.H * 4, hipMemcpyHostToDevice));
    int zero = 0;
    uint32_t sb = seed_bits(dv->par.seed);
    CK(hipMemcpy(dv->cur_row, &zero, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv->stopped, &zero, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv->st_rng, &sb, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv->codes, &first_code, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv->last_tok, &first_code, 4, hipMemcpyHostToDevice));
    dv->nrun = 1;
    int rc = subtalker(dv);
    dv->nrun = dv->nb;
    CKI(rc);
    CK(hipMemcpyAsync(out_codes, dv->codes, (size_t)d.G * 4, hipMemcpyDeviceToHost, dv->st));
    CK(hipStreamSynchronize(dv->st));
    return 0;
}
