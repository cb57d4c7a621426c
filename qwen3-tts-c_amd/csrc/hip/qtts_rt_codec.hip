// qtts_rt_codec.hip - the codec entries of the C-ABI (include/qtts_hip.h):
// one-shot decode of a slot or of host codes, the exact stream, the
// multi-stream with its snapshots, the decode overlapped on a second stream
// and a batch's passes side by side.  Each only drives CodecModel
// (k_codec.hip) with the context's codes, streams and staging buffers.
#include "qtts_dev.h"

extern "C" float *qtts_dev_codec_slot(qtts_dev_t *dv, int b, int T, int *out_samples) {
    if (out_samples) *out_samples = 0;
    if (!dv || b < 0 || b >= dv->nb || T < 1) return nullptr;
    hipSetDevice(dv->device);
    if (join_prime(dv)) return nullptr;   // the prime shares the codec scratch and split-K workspace
    return codec_decode(&dv->codec, dv->codes + (size_t)b * (dv->max_frames + 1) * dv->d.G, T, out_samples);
}

extern "C" int qtts_dev_codec_timing(qtts_dev_t *dv, int on) {
    if (!dv) return -1;
    dv->codec.timing = on != 0;
    return 0;
}

extern "C" int qtts_dev_codec_stage_ms(const qtts_dev_t *dv, float *ms) {
    if (!dv || !ms || !dv->codec.timed) return -1;
    for (int i = 0; i < 5; ++i) ms[i] = dv->codec.stage_ms[i];
    return 0;
}

// ----------------------------------------------------------------- streaming codec (exact, incremental)
// a pending prime (below) orders every later use of the stream state after it
int join_prime(qtts_dev *dv) {
    if (!dv->prime_pending) return 0;
    dv->prime_pending = false;
    CK(hipStreamWaitEvent(dv->st, dv->cev, 0));
    return 0;
}

static int ensure_cst(qtts_dev *dv) {
    if (dv->cst) return 0;
    int lo = 0, hi = 0;
    CK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CK(hipStreamCreateWithPriority(&dv->cst, hipStreamNonBlocking, lo));   // lowest: the decode goes first
    CK(hipEventCreateWithFlags(&dv->cev, hipEventDisableTiming));
    return 0;
}

static int ensure_push_codes(qtts_dev *dv, size_t n) {
    if (n <= dv->push_cap) return 0;
    CK(hipDeviceSynchronize());
    if (dv->push_codes) CK(hipFree(dv->push_codes));
    dv->push_codes = nullptr;
    dv->push_cap = 0;
    const size_t cap = n < 4096 ? 4096 : n;
    CK(hipMalloc(&dv->push_codes, cap * 4));
    dv->push_cap = cap;
    return 0;
}

extern "C" int qtts_dev_codec_stream_begin(qtts_dev_t *dv, int max_frames) {
    return qtts_dev_codec_stream_begin_ex(dv, max_frames, 0);
}

extern "C" int qtts_dev_codec_stream_begin_ex(qtts_dev_t *dv, int max_frames, int chunk_frames) {
    if (!dv || max_frames < 1) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    CK(hipStreamSynchronize(dv->st));
    return codec_stream_begin(&dv->codec, max_frames, chunk_frames);
}

// Push T host frames through the stream on the second stream (cst) without
// waiting: their audio is dropped (device scratch), the carried state is what
// later pushes continue from.  The voice-clone reference frames go this way
// while the prefill runs on the context stream (SURVEY.md 8f N1 + N2).
extern "C" int qtts_dev_codec_stream_prime(qtts_dev_t *dv, const int *codes, int T) {
    if (!dv || !codes || T < 1) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    CKI(ensure_cst(dv));
    CKI(ensure_push_codes(dv, (size_t)T * dv->d.cq));
    const size_t need = (size_t)T * 1920;
    if (need > dv->pwav_cap) {
        CK(hipStreamSynchronize(dv->cst));
        if (dv->pwav) CK(hipFree(dv->pwav));
        dv->pwav = nullptr;
        dv->pwav_cap = 0;
        CK(hipMalloc(&dv->pwav, need * 4));
        dv->pwav_cap = need;
    }
    CK(hipEventRecord(dv->cev, dv->st));          // after the begin's resets on st
    CK(hipStreamWaitEvent(dv->cst, dv->cev, 0));
    CK(hipMemcpyAsync(dv->push_codes, codes, (size_t)T * dv->d.cq * 4, hipMemcpyHostToDevice, dv->cst));
    dv->codec.st = dv->cst;
    const int n = codec_stream_push_to(&dv->codec, dv->push_codes, dv->d.cq, T, dv->pwav, false);
    dv->codec.st = dv->st;
    if (n < 0) return -1;
    CK(hipEventRecord(dv->cev, dv->cst));
    dv->prime_pending = true;
    return 0;
}

extern "C" int qtts_dev_codec_stream_push_slot(qtts_dev_t *dv, int b, int frame0, int T, float *host_out) {
    if (!dv || b < 0 || b >= dv->nb || T < 1 || frame0 < 0 || frame0 + T > dv->max_frames + 1) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    const int *codes = dv->codes + (size_t)b * (dv->max_frames + 1) * dv->d.G + (size_t)frame0 * dv->d.G;
    return codec_stream_push(&dv->codec, codes, dv->d.G, T, host_out);
}

extern "C" int qtts_dev_codec_stream_push_host(qtts_dev_t *dv, const int *codes, int T, float *host_out) {
    if (!dv || !codes || T < 1) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    const size_t n = (size_t)T * dv->d.cq;
    CKI(ensure_push_codes(dv, n));   // persistent staging buffer: no allocation per push
    // ordered on the codec's stream before the push reads it; the synchronous
    // push waits for the stream before returning, so the host buffer may be reused
    CK(hipMemcpyAsync(dv->push_codes, codes, n * 4, hipMemcpyHostToDevice, dv->codec.st));
    return codec_stream_push(&dv->codec, dv->push_codes, dv->d.cq, T, host_out);
}

// ----------------------------------------------------------------- multi-stream codec (n exact streams, one pass)
extern "C" int qtts_dev_codec_mstream_begin(qtts_dev_t *dv, int n_streams, int max_frames, int chunk_frames) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    CK(hipStreamSynchronize(dv->st));
    return codec_mstream_begin(&dv->codec, n_streams, max_frames, chunk_frames);
}

// One push of n streams, behind the seven entries below.  The codes come from
// the slots' generated frames on the device or from host codes staged on the
// codec's stream; every stream advances by T frames or stream i by counts[i]
// (ragged: one launch sequence per pass whatever the counts, DESIGN.md 7,
// "Ragged pushes"); `any`: the streams may stand at independent positions (the
// work queue's slots: a refilled slot's stream restarts at 0 beside its
// neighbours; a ragged push always may).  A prime is the ragged host push on
// the second stream (cst), its audio dropped, not waited for: the carried state
// is what later pushes continue from.  The reference frames of a voice-clone
// batch go this way while the prefill runs on the context stream, as
// qtts_dev_codec_stream_prime's do for one utterance; every later multi-stream
// call joins it by event.
enum MsSrc { MS_SLOTS, MS_SLOTS_AT, MS_HOST };
struct MsPush {
    MsSrc src;
    const int *slots;      // MS_SLOTS / MS_SLOTS_AT: slot slots[i]'s frames from
    int frame0;            //   MS_SLOTS: frame0, the same for every stream
    const int *frame0s;    //   MS_SLOTS_AT: frame0s[i]
    const int *codes;      // MS_HOST: [n][ld][16], stream i's first T / counts[i] rows
    int ld;
    bool ragged;
    const int *counts;
    int T;
    bool any;
    bool prime;
};

static int mstream_push(qtts_dev_t *dv, int n, const int *streams, const MsPush &p, float *const *host_out) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    const int cap = dv->max_frames + 1;   // frames a slot holds
    // every refusal before anything is enqueued
    if (p.ragged ? codec_mstream_check_ragged(&dv->codec, n, streams, p.counts, p.src == MS_HOST ? p.ld : cap)
                 : codec_mstream_check(&dv->codec, n, streams, p.T, p.any))
        return -1;
    if (p.src == MS_HOST) {
        if (!p.codes || (!p.prime && !host_out)) return -1;
    } else if (p.src == MS_SLOTS) {
        if (!p.slots || !host_out || p.frame0 < 0 || p.frame0 + p.T > cap) {
            fprintf(stderr, "qtts codec mstream: frames [%d, %d) are outside the slots' %d\n", p.frame0,
                    p.frame0 + p.T, cap);
            return -1;
        }
    } else if (!p.slots || !p.frame0s || !host_out) {
        return -1;
    }
    const size_t per = (size_t)(p.ragged ? p.ld : p.T) * dv->d.cq;   // MS_HOST: the staged codes of one stream
    long long off[64];   // (the check bounds n by the begin's 1..64 streams)
    for (int i = 0; i < n; ++i) {
        if (p.ragged && !p.prime && !host_out[i]) return -1;
        if (p.src == MS_HOST) {
            off[i] = (long long)(i * per);
            continue;
        }
        if (p.slots[i] < 0 || p.slots[i] >= dv->nb) {
            fprintf(stderr, "qtts codec mstream: slot %d out of range (0..%d)\n", p.slots[i], dv->nb - 1);
            return -1;
        }
        const int f0 = p.src == MS_SLOTS ? p.frame0 : p.frame0s[i], c = p.ragged ? p.counts[i] : p.T;
        if (f0 < 0 || f0 + c > cap) {   // (MS_SLOTS: refused above for all)
            fprintf(stderr, "qtts codec mstream: frames [%d, %d) are outside slot %d's %d\n", f0, f0 + c, p.slots[i],
                    cap);
            return -1;
        }
        off[i] = ((long long)p.slots[i] * cap + f0) * dv->d.G;
    }
    CKI(join_prime(dv));
    const int *base = dv->codes;
    int ldc = dv->d.G;
    if (p.src == MS_HOST) {
        if (p.prime) CKI(ensure_cst(dv));
        CKI(ensure_push_codes(dv, per * n));   // persistent staging buffer: no allocation per push
        if (p.prime) {
            CK(hipEventRecord(dv->cev, dv->st));          // after the begin's resets on st
            CK(hipStreamWaitEvent(dv->cst, dv->cev, 0));
        }
        // ordered on the codec's stream before the push reads it
        CK(hipMemcpyAsync(dv->push_codes, p.codes, per * n * 4, hipMemcpyHostToDevice, p.prime ? dv->cst : dv->codec.st));
        base = dv->push_codes;
        ldc = dv->d.cq;
    }
    if (p.prime) dv->codec.st = dv->cst;
    const int r = p.ragged ? codec_mstream_push_ragged(&dv->codec, n, streams, base, off, ldc, p.counts,
                                                       p.prime ? nullptr : host_out)
                           : codec_mstream_push(&dv->codec, n, streams, base, off, ldc, p.T, host_out, p.any);
    if (!p.prime) return r;
    dv->codec.st = dv->st;
    if (r < 0) return -1;
    CK(hipEventRecord(dv->cev, dv->cst));
    dv->prime_pending = true;
    return 0;
}

extern "C" int qtts_dev_codec_mstream_push_slots(qtts_dev_t *dv, int n, const int *streams, const int *slots,
                                                 int frame0, int T, float *const *host_out) {
    MsPush p{};
    p.src = MS_SLOTS; p.slots = slots; p.frame0 = frame0; p.T = T;
    return mstream_push(dv, n, streams, p, host_out);
}

extern "C" int qtts_dev_codec_mstream_push_host(qtts_dev_t *dv, int n, const int *streams, const int *codes, int T,
                                                float *const *host_out) {
    MsPush p{};
    p.src = MS_HOST; p.codes = codes; p.T = T;
    return mstream_push(dv, n, streams, p, host_out);
}

extern "C" int qtts_dev_codec_mstream_push_slots_at(qtts_dev_t *dv, int n, const int *streams, const int *slots,
                                                    const int *frame0, int T, float *const *host_out) {
    MsPush p{};
    p.src = MS_SLOTS_AT; p.slots = slots; p.frame0s = frame0; p.T = T; p.any = true;
    return mstream_push(dv, n, streams, p, host_out);
}

extern "C" int qtts_dev_codec_mstream_push_host_any(qtts_dev_t *dv, int n, const int *streams, const int *codes, int T,
                                                    float *const *host_out) {
    MsPush p{};
    p.src = MS_HOST; p.codes = codes; p.T = T; p.any = true;
    return mstream_push(dv, n, streams, p, host_out);
}

// counts[i] * 1920 samples reach host_out[i]; returns the largest count times 1920
extern "C" int qtts_dev_codec_mstream_push_host_ragged(qtts_dev_t *dv, int n, const int *streams, const int *codes,
                                                       const int *counts, int ld_frames, float *const *host_out) {
    MsPush p{};
    p.src = MS_HOST; p.codes = codes; p.ld = ld_frames; p.ragged = true; p.counts = counts;
    return mstream_push(dv, n, streams, p, host_out);
}

extern "C" int qtts_dev_codec_mstream_push_slots_ragged(qtts_dev_t *dv, int n, const int *streams, const int *slots,
                                                        const int *frame0, const int *count,
                                                        float *const *host_out) {
    MsPush p{};
    p.src = MS_SLOTS_AT; p.slots = slots; p.frame0s = frame0; p.ragged = true; p.counts = count;
    return mstream_push(dv, n, streams, p, host_out);
}

extern "C" int qtts_dev_codec_mstream_prime(qtts_dev_t *dv, int n, const int *streams, const int *codes,
                                            const int *counts, int ld_frames) {
    MsPush p{};
    p.src = MS_HOST; p.codes = codes; p.ld = ld_frames; p.ragged = true; p.counts = counts; p.prime = true;
    return mstream_push(dv, n, streams, p, nullptr);
}

extern "C" int qtts_dev_codec_mstream_reset(qtts_dev_t *dv, int stream) {
    if (!dv) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));   // a pending prime owns the histories until joined
    return codec_mstream_reset(&dv->codec, stream);
}

extern "C" int qtts_dev_codec_mstream_pos(qtts_dev_t *dv, int stream) {
    if (!dv) return -1;
    return codec_mstream_pos(&dv->codec, stream);
}

static std::mutex g_snaps_mu;
static std::set<const qtts_codec_snapshot_t *> g_snaps;

void snapshots_orphan(qtts_dev *dv) {
    std::lock_guard<std::mutex> lk(g_snaps_mu);
    for (qtts_codec_snapshot_t *p : dv->snaps) {
        codec_snapshot_release(&p->s);
        p->owner = nullptr;
    }
    dv->snaps.clear();
}

// One stream's carried state saved and restored ("Snapshots").
// Both are one launch on the context stream after a pending prime is joined,
// and wait for nothing on the host.
extern "C" qtts_codec_snapshot_t *qtts_dev_codec_mstream_save(qtts_dev_t *dv, int stream) {
    if (!dv) return nullptr;
    hipSetDevice(dv->device);
    if (join_prime(dv)) return nullptr;
    qtts_codec_snapshot_t *p = new qtts_codec_snapshot_t();
    if (codec_mstream_save(&dv->codec, stream, &p->s)) {
        delete p;
        return nullptr;
    }
    p->owner = dv;
    std::lock_guard<std::mutex> lk(g_snaps_mu);
    g_snaps.insert(p);
    dv->snaps.push_back(p);
    return p;
}

extern "C" int qtts_dev_codec_mstream_restore(qtts_dev_t *dv, int stream, const qtts_codec_snapshot_t *snap) {
    if (!dv) return -1;
    {
        std::lock_guard<std::mutex> lk(g_snaps_mu);
        if (!snap || !g_snaps.count(snap)) {
            fprintf(stderr, "qtts codec mstream: restore takes a live snapshot (got %s)\n",
                    snap ? "a freed one" : "NULL");
            return -1;
        }
        if (snap->owner != dv) {
            fprintf(stderr, "qtts codec mstream: restore: the snapshot belongs to %s\n",
                    snap->owner ? "another context" : "a context that was freed");
            return -1;
        }
    }
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    return codec_mstream_restore(&dv->codec, stream, &snap->s);
}

extern "C" void qtts_dev_codec_snapshot_free(qtts_codec_snapshot_t *snap) {
    std::lock_guard<std::mutex> lk(g_snaps_mu);
    if (!snap || !g_snaps.count(snap)) return;
    g_snaps.erase(snap);
    if (qtts_dev *dv = snap->owner) {
        hipSetDevice(dv->device);
        hipStreamSynchronize(dv->st);   // a restore that reads it may still be queued
        if (dv->cst) hipStreamSynchronize(dv->cst);
        dv->snaps.erase(std::remove(dv->snaps.begin(), dv->snaps.end(), snap), dv->snaps.end());
        codec_snapshot_release(&snap->s);
    }
    delete snap;
}

extern "C" int qtts_dev_codec_snapshot_pos(const qtts_codec_snapshot_t *snap) {
    std::lock_guard<std::mutex> lk(g_snaps_mu);
    if (!snap || !g_snaps.count(snap) || !snap->owner) return -1;
    return snap->s.pos0;
}

extern "C" long long qtts_dev_codec_snapshot_bytes(const qtts_codec_snapshot_t *snap) {
    std::lock_guard<std::mutex> lk(g_snaps_mu);
    if (!snap || !g_snaps.count(snap) || !snap->owner) return -1;
    return (long long)snap->s.elems * 4;
}

// ----------------------------------------------------------------- codec overlapped with the decode
// The exact streaming decode (codec_stream_*), run on a second stream while
// the frame graphs continue on the context stream: each push waits (event)
// for the frames already enqueued, decodes them into a device waveform, and
// nothing is waited for on the host until qtts_dev_codec_async_end.
extern "C" int qtts_dev_codec_async_begin(qtts_dev_t *dv, int max_frames) {
    if (!dv || max_frames < 1) return -1;
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    CKI(ensure_cst(dv));
    const size_t need = (size_t)max_frames * 1920;
    if (need > dv->cwav_cap) {
        CK(hipStreamSynchronize(dv->cst));
        if (dv->cwav) CK(hipFree(dv->cwav));
        dv->cwav = nullptr;
        CK(hipMalloc(&dv->cwav, need * 4));
        dv->cwav_cap = need;
    }
    CK(hipStreamSynchronize(dv->st));   // the stream state is shared with the synchronous paths
    dv->codec.st = dv->cst;
    const int rc = codec_stream_begin(&dv->codec, max_frames);
    dv->codec.st = dv->st;
    return rc;
}

extern "C" int qtts_dev_codec_async_push(qtts_dev_t *dv, int b, int frame0, int T) {
    if (!dv || !dv->cst || b < 0 || b >= dv->nb || T < 1 || frame0 < 0 || frame0 + T > dv->max_frames + 1 ||
        (size_t)(frame0 + T) * 1920 > dv->cwav_cap)
        return -1;
    hipSetDevice(dv->device);
    CK(hipEventRecord(dv->cev, dv->st));
    CK(hipStreamWaitEvent(dv->cst, dv->cev, 0));
    const int *codes = dv->codes + (size_t)b * (dv->max_frames + 1) * dv->d.G + (size_t)frame0 * dv->d.G;
    dv->codec.st = dv->cst;
    const int n = codec_stream_push_to(&dv->codec, codes, dv->d.G, T, dv->cwav + (size_t)frame0 * 1920, false);
    dv->codec.st = dv->st;
    return n;
}

extern "C" int qtts_dev_codec_async_end(qtts_dev_t *dv, float *host_out, int frames) {
    if (!dv || !dv->cst || frames < 0 || (size_t)frames * 1920 > dv->cwav_cap) return -1;
    hipSetDevice(dv->device);
    if (frames > 0)
        CK(hipMemcpyAsync(host_out, dv->cwav, (size_t)frames * 1920 * 4, hipMemcpyDeviceToHost, dv->cst));
    CK(hipStreamSynchronize(dv->cst));
    return frames * 1920;
}

extern "C" float *qtts_dev_codec_decode_host(qtts_dev_t *dv, const int *codes, int T, int *out_samples) {
    if (out_samples) *out_samples = 0;
    if (!dv || T < 1) return nullptr;
    hipSetDevice(dv->device);
    if (join_prime(dv)) return nullptr;
    int *dc = nullptr;
    if (hipMalloc(&dc, (size_t)T * dv->d.cq * 4) != hipSuccess) return nullptr;
    float *r = nullptr;
    if (hipMemcpy(dc, codes, (size_t)T * dv->d.cq * 4, hipMemcpyHostToDevice) == hipSuccess)
        r = codec_decode(&dv->codec, dc, T, out_samples);
    hipFree(dc);
    return r;
}

// Several utterances' codec passes at once (a batch's slots, run_batch): job
// i decodes host_codes[i] (T[i] frames, [T][cq] time-major) when given, else
// slot slot[i]'s first T[i] generated frames.  QTTS_HIP_CODEC_LANES (default
// 8, fewer when the extra lanes' scratch would pass 16 GB) passes run side by
// side (codec_decode_many); 1 decodes them one after another with
// codec_decode.  audio[i] is malloc'd host memory.  Measured (1.7B, 128
// frames, profiles/r05lm_ab_codec_lanes.txt): a batch of 8's codec 73.4 ->
// 60.7 ms, of 16 146.8 -> 120.0 ms (the passes are mostly conv throughput).
extern "C" int qtts_dev_codec_multi(qtts_dev_t *dv, int n, const int *const *host_codes, const int *slot, const int *T,
                                    float **audio, int *samples) {
    if (!dv || n < 1 || !T || !audio || !samples) return -1;
    for (int i = 0; i < n; ++i) {
        audio[i] = nullptr;
        samples[i] = 0;
        const bool host = host_codes && host_codes[i];
        if (T[i] < 1 || (!host && (!slot || slot[i] < 0 || slot[i] >= dv->nb || T[i] > dv->max_frames + 1)))
            return -1;
    }
    hipSetDevice(dv->device);
    CKI(join_prime(dv));
    const int cq = dv->d.cq;
    // host codes staged once for every job
    size_t nh = 0;
    for (int i = 0; i < n; ++i)
        if (host_codes && host_codes[i]) nh += (size_t)T[i] * cq;
    if (nh > dv->mcodes_cap) {
        CK(hipDeviceSynchronize());
        if (dv->mcodes) CK(hipFree(dv->mcodes));
        dv->mcodes = nullptr;
        dv->mcodes_cap = 0;
        CK(hipMalloc(&dv->mcodes, nh * 4));
        dv->mcodes_cap = nh;
    }
    std::vector<const int *> dcodes(n);
    size_t ho = 0;
    for (int i = 0; i < n; ++i) {
        if (host_codes && host_codes[i]) {
            CK(hipMemcpyAsync(dv->mcodes + ho, host_codes[i], (size_t)T[i] * cq * 4, hipMemcpyHostToDevice, dv->st));
            dcodes[i] = dv->mcodes + ho;
            ho += (size_t)T[i] * cq;
        } else {
            dcodes[i] = dv->codes + (size_t)slot[i] * (dv->max_frames + 1) * dv->d.G;
        }
    }
    const char *e = getenv("QTTS_HIP_CODEC_LANES");
    int nl = e ? atoi(e) : 8;
    if (nl < 1) nl = 1;
    if (nl > 16) nl = 16;
    if (nl > n) nl = n;
    // the extra lanes' scratch within 16 GB (a 128-frame decode state is ~0.4 GB,
    // a 4096-frame one ~12 GB: long EOS utterances decode on fewer lanes)
    int tmax = 1;
    for (int i = 0; i < n; ++i) tmax = T[i] > tmax ? T[i] : tmax;
    const size_t per_lane = codec_state_bytes(&dv->codec, tmax);
    while (nl > 1 && (size_t)(nl - 1) * per_lane > ((size_t)16 << 30)) --nl;
    auto fail = [&]() {
        for (int i = 0; i < n; ++i) {
            free(audio[i]);
            audio[i] = nullptr;
            samples[i] = 0;
        }
        return -1;
    };
    if (nl == 1) {
        for (int i = 0; i < n; ++i) {
            audio[i] = codec_decode(&dv->codec, dcodes[i], T[i], &samples[i]);
            if (!audio[i]) return fail();
        }
        return 0;
    }
    while ((int)dv->clanes.size() < nl - 1) {
        hipStream_t st = nullptr;
        CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        dv->clane_st.push_back(st);
        dv->clanes.push_back(codec_lane_new(&dv->codec, st));
    }
    std::vector<CodecModel *> lanes(nl, nullptr);
    for (int k = 1; k < nl; ++k) lanes[k] = dv->clanes[k - 1];
    // one hop of samples per frame: the decoder's total upsampling (2 x 2 x 8 x
    // 5 x 4 x 3 = 1920 for the released codec), exactly codec_decode's L / T
    const size_t hop = (size_t)dv->d.ratios[0] * dv->d.ratios[1] * dv->d.rates[0] * dv->d.rates[1] *
                       dv->d.rates[2] * dv->d.rates[3];
    std::vector<size_t> off(n);
    size_t tot = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = tot;
        tot += (size_t)T[i] * hop;
    }
    if (tot > dv->mwav_cap) {
        CK(hipDeviceSynchronize());
        if (dv->mwav) CK(hipFree(dv->mwav));
        dv->mwav = nullptr;
        dv->mwav_cap = 0;
        CK(hipMalloc(&dv->mwav, tot * 4));
        dv->mwav_cap = tot;
    }
    std::vector<int> ns(n, 0);
    if (codec_decode_many(&dv->codec, lanes.data(), nl, n, dcodes.data(), T, dv->mwav, off.data(), ns.data()))
        return fail();
    for (int i = 0; i < n; ++i) {
        if ((size_t)ns[i] != (size_t)T[i] * hop) return fail();
        audio[i] = (float *)malloc((size_t)ns[i] * sizeof(float));
        if (!audio[i] ||
            hipMemcpy(audio[i], dv->mwav + off[i], (size_t)ns[i] * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail();
        samples[i] = ns[i];
    }
    return 0;
}
