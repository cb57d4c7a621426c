// qtts_argdump.h - the arguments of every launcher entry as text, one line per
// call, for an argument-for-argument comparison of two builds
// (tools/frame_args_ab.py).  Compiled only with `make EXTRA=-DQTTS_ARGDUMP`
// (qtts_kernels.h includes it under that macro; the product build holds none
// of it).  A line goes to the file QTTS_ARGDUMP_FILE names (appended; unset:
// nothing is written): the entry's name, every scalar field, then every
// pointer as p<k>, k = the order of first appearance of that address in the
// process (p- for a null pointer), so two runs that pass the same buffers in
// the same roles write the same lines whatever the allocator returned.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <mutex>
#include <string>

namespace qtts_argdump {

struct State {
    std::mutex mu;
    std::map<const void *, int> ids;
    FILE *f = nullptr;
    State() {
        const char *p = getenv("QTTS_ARGDUMP_FILE");
        if (p && *p) f = fopen(p, "a");
    }
};
inline State &state() {
    static State s;
    return s;
}

// one line under construction; written when it goes out of scope
struct Line {
    std::string s;
    explicit Line(const char *name) : s(name) {}
    Line &i(const char *k, long long v) {
        char b[64];
        snprintf(b, sizeof b, " %s=%lld", k, v);
        s += b;
        return *this;
    }
    Line &f(const char *k, double v) {
        char b[64];
        snprintf(b, sizeof b, " %s=%.9g", k, v);
        s += b;
        return *this;
    }
    Line &p(const char *k, const void *v) {   // (under the lock: the ids are handed out in call order)
        char b[64];
        if (!v) snprintf(b, sizeof b, " %s=p-", k);
        else {
            State &st = state();
            auto it = st.ids.find(v);
            if (it == st.ids.end()) it = st.ids.emplace(v, (int)st.ids.size()).first;
            snprintf(b, sizeof b, " %s=p%d", k, it->second);
        }
        s += b;
        return *this;
    }
    Line &pf(const L2Prefetch &q) {
        i("pf.pm", q.pm).i("pf.pa", q.pa).i("pf.pb", q.pb).i("pf.chunks", q.chunks).i("pf.lg", q.lg).i("pf.ld", q.ld);
        return i("pf.cs", q.cs).i("pf.nwg", q.nwg).p("pf.base", q.base).p("pf.sink", q.sink);
    }
    ~Line() {
        State &st = state();
        if (!st.f) return;
        fprintf(st.f, "%s\n", s.c_str());
        fflush(st.f);
    }
};
struct Lock {   // a whole line (its pointer ids and its write) is one step
    std::lock_guard<std::mutex> g;
    Lock() : g(state().mu) {}
};

inline void gemv(const char *name, const GemvArgs &a, long long extra = 0, const void *x0 = nullptr, const void *x1 = nullptr,
                 const void *x2 = nullptr) {
    Lock lk;
    Line l(name);
    l.i("R", a.R).i("C", a.C).i("ksplit", a.ksplit).i("cch", a.cch).i("nt", a.nt).i("nb", a.nb).i("ldx", a.ldx);
    l.i("ids_bstride", a.ids_bstride).i("ids_rstride", a.ids_rstride).i("ids_off", a.ids_off).i("reps", a.reps);
    l.i("ldy_rep", (long long)a.ldy_rep).i("n_xadd", a.n_xadd).i("ld_xadd", a.ld_xadd).i("ldb_xadd", a.ldb_xadd);
    l.i("am_nsplit", a.am_nsplit).i("am_ch", a.am_ch).i("am_hd", a.am_hd).i("am_gph", a.am_gph);
    l.i("ld_ypart", (long long)a.ld_ypart).i("kz", a.kz).f("eps", a.eps).i("ldxc", a.ldxc).i("xcopy_normed", a.xcopy_normed);
    l.i("ldy", a.ldy).i("epi", a.epi).i("extra", extra);
    l.p("W", a.W).p("x", a.x).p("table", a.table).p("table_f32", a.table_f32).p("ids", a.ids).p("row_sel", a.row_sel);
    l.p("xadd", a.xadd).p("amerge", a.amerge).p("am_pos", a.am_pos).p("ypart", a.ypart).p("tick", a.tick);
    l.p("norm_w", a.norm_w).p("xcopy", a.xcopy).p("y", a.y).p("bias", a.bias).p("dbg", a.dbg);
    l.p("x0", x0).p("x1", x1).p("x2", x2).pf(a.pf);
}

inline void attn(const char *name, const AttnArgs &a, long long extra = 0, const void *x0 = nullptr, const void *x1 = nullptr) {
    Lock lk;
    Line l(name);
    l.i("mode", a.mode).i("ld_qkv", a.ld_qkv).f("eps", a.eps).i("S", a.S).i("pos_const", a.pos_const).i("NH", a.NH);
    l.i("KV", a.KV).i("HD", a.HD).i("ld_out", a.ld_out).i("nrows", a.nrows).i("win", a.win).i("tab_bstride", a.tab_bstride);
    l.i("tab_rstride", a.tab_rstride).i("tab_off", a.tab_off).i("nsplit", a.nsplit).i("defer", a.defer).i("xc_n", a.xc_n);
    l.i("lpk", a.lpk).i("kv_dtype", a.kv_dtype).i("extra", extra);
    l.p("qkv", a.qkv).p("qn_w", a.qn_w).p("kn_w", a.kn_w).p("rope_cos", a.rope_cos).p("rope_sin", a.rope_sin);
    l.p("kc", a.kc).p("vc", a.vc).p("pos", a.pos).p("row_b", a.row_b).p("out", a.out).p("skip", a.skip);
    l.p("qkv_tab", a.qkv_tab).p("tab_ids", a.tab_ids).p("tab_row_sel", a.tab_row_sel).p("part", a.part).p("cnt", a.cnt);
    l.p("xc_tab", a.xc_tab).p("xc_tab16", a.xc_tab16).p("xc_dst", a.xc_dst).p("x0", x0).p("x1", x1).pf(a.pf);
}

inline void samp(const char *name, const SampArgs &a, long long extra = 0, const void *x0 = nullptr, const void *x1 = nullptr,
                 const SampForce *fo = nullptr) {
    Lock lk;
    Line l(name);
    l.i("ld", a.ld).i("n", a.n).i("nb", a.nb).i("top_k", a.top_k).f("top_p", a.top_p).f("temp", a.temp).i("mode", a.mode);
    l.i("suppress_lo", a.suppress_lo).i("eos", a.eos).f("rep", a.rep).i("fixed", a.fixed).i("seed_bits", a.seed_bits);
    l.i("codes_bstride", a.codes_bstride).i("G", a.G).i("g", a.g).i("extra", extra).i("tap_ld", fo ? fo->tap_ld : 0);
    l.p("logits", a.logits).p("rng", a.rng).p("counts", a.counts).p("n_gen", a.n_gen).p("stopped", a.stopped);
    l.p("cur_row", a.cur_row).p("stop_step", a.stop_step).p("host_stopped", a.host_stopped).p("st_rng", a.st_rng);
    l.p("codes", a.codes).p("out_tok", a.out_tok).p("x0", x0).p("x1", x1);
    if (fo) l.p("forced", fo->forced).p("drawn", fo->drawn).p("taps", fo->taps).p("tap_logits", fo->tap_logits).p("tap_meta", fo->tap_meta);
}

inline void embed(const char *name, const EmbedSumArgs &a) {
    Lock lk;
    Line l(name);
    l.i("codes_bstride", a.codes_bstride).i("G", a.G).i("Vs", a.Vs).i("H", a.H).i("nb", a.nb).i("tr_cap", a.tr_cap);
    l.i("advance", a.advance);
    l.p("codes", a.codes).p("cur_row", a.cur_row).p("stopped", a.stopped).p("codec_emb", a.codec_emb).p("st_emb", a.st_emb);
    l.p("trailing", a.trailing).p("n_trailing", a.n_trailing).p("pad", a.pad).p("out", a.out).p("kv_len", a.kv_len);
}

}  // namespace qtts_argdump
