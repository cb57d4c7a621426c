// k_sample_p.hip - the sampler's per-slot form (qtts_dev_slot_params; the row
// layout in qtts_kernels.h SampSlotRow, the device code in qtts_sample_dev.h
// sample_row_p): workgroup b draws with row b of the parameter table
// instead of the launch's arguments.  A file of its own, as k_sample_f.hip is,
// so that k_sample.hip's and k_sample_f.hip's objects -- the kernels every
// unarmed and every forced run launches -- stay what they were.
//
// Fast or full is a property of the row, so there are two families:
//   k_sample_pw<EM>  1024 threads, fast path only (k_sample_w's analogue): for
//                    runs whose every row is fast-path eligible in both modes
//   k_sample_p<EM>   256 threads, KSmem: fast or full per row, a
//                    workgroup-uniform branch; also the QTTS_HIP_SAMPLE_W=0 form
// The caller (the run, qtts_runtime.hip) says which: a row that needs the full
// path never reaches the fast-only kernel.
#include <atomic>
#include "qtts_sample_dev.h"

namespace {

template <int EM>
__global__ __launch_bounds__(256) void k_sample_p(SampArgs a, const SampSlotRow *tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row_p<false, EM, 256>(a, tab, blockIdx.x, smraw, a.logits, a.stopped,
                                            a.mode == 1 ? a.rng : a.st_rng, a.n_gen, a.counts);
}

// the table and the row's input pointers lead the arguments (preloaded into
// SGPRs, Makefile)
template <int EM>
__global__ __launch_bounds__(1024) void k_sample_pw(const SampSlotRow *tab, const float *logits, const int *stopped,
                                                    const uint32_t *rng, const int *n_gen, const int *counts,
                                                    SampArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row_p<true, EM, 1024>(a, tab, blockIdx.x, smraw, logits, stopped, rng, n_gen, counts);
}

// a fed run's general form: the row reads the gate, the EOS goes to a.stopped
template <int EM>
__global__ __launch_bounds__(256) void k_sample_pg(const int *stop_rd, SampArgs a, const SampSlotRow *tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row_p<false, EM, 256>(a, tab, blockIdx.x, smraw, a.logits, stop_rd,
                                            a.mode == 1 ? a.rng : a.st_rng, a.n_gen, a.counts);
}

std::atomic<long long> g_slot_launches{0};

}  // namespace

// per-slot sampler launches enqueued (or captured) since the library loaded
long long qtts_sample_slot_launches() { return g_slot_launches.load(); }

// one table row, stream-ordered (the values travel as kernel arguments, so no
// host buffer has to outlive the call); rng / st_rng non-null: the slot's RNG
// states start from the row's seed as well
namespace {
__global__ void k_slot_row_set(SampSlotRow *tab, int b, SampSlotRow r, uint32_t *rng, uint32_t *st_rng) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    tab[b] = r;
    if (rng) rng[b] = r.seed_bits;
    if (st_rng) st_rng[b] = r.seed_bits;
}
}  // namespace
int qtts_slot_row_set(SampSlotRow *tab, int b, const SampSlotRow &r, uint32_t *rng, uint32_t *st_rng, hipStream_t st) {
    hipLaunchKernelGGL(k_slot_row_set, dim3(1), dim3(64), 0, st, tab, b, r, rng, st_rng);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

bool qtts_sample_row_fast(const SampSlotRow &r, int mode, int n) {
    return mode == 1 ? qtts_samp::fast_path_row(r.top_p, r.top_k, n) : qtts_samp::fast_path_row(r.st_top_p, r.st_top_k, n);
}

int qtts_sample_slots(const SampArgs &a, const SampSlotRow *tab, bool all_fast, hipStream_t st, const int *stop_rd) {
#ifdef QTTS_ARGDUMP
    qtts_argdump::samp("qtts_sample_slots", a, all_fast, stop_rd, tab);
#endif
    if (a.n > qtts_samp::NMAX || a.n < 1) {
        fprintf(stderr, "qtts_sample: vocab %d unsupported (max %d)\n", a.n, qtts_samp::NMAX);
        return -1;
    }
    if (!tab) {
        fprintf(stderr, "qtts_sample_slots: no parameter table\n");
        return -1;
    }
    // QTTS_HIP_SAMPLE_W=0: every row on the 256-thread kernel (read per call, as qtts_sample does)
    const char *sw = getenv("QTTS_HIP_SAMPLE_W");
    if (all_fast && !(sw && !atoi(sw))) {
        const size_t sm = sizeof(qtts_samp::FastSmemNT<1024>);
        const uint32_t *rng = a.mode == 1 ? a.rng : a.st_rng;
        const int *rd = stop_rd ? stop_rd : (const int *)a.stopped;
        if (a.n <= 2 * 1024) {
            hipLaunchKernelGGL((k_sample_pw<2>), dim3(a.nb), dim3(1024), sm, st, tab, a.logits, rd,
                               rng, (const int *)a.n_gen, (const int *)a.counts, a);
            qtts_last_kernel = "k_sample_pw<2>";
        } else {
            hipLaunchKernelGGL((k_sample_pw<4>), dim3(a.nb), dim3(1024), sm, st, tab, a.logits, rd,
                               rng, (const int *)a.n_gen, (const int *)a.counts, a);
            qtts_last_kernel = "k_sample_pw<4>";
        }
    } else if (qtts_sample_nucleus_on()) {
        // fast, nucleus short list or full per row (k_sample_n.hip; QTTS_HIP_SAMPLE_NUCLEUS=0: the kernels below)
        if (qtts_sample_slots_n(a, tab, st, stop_rd, nullptr, true) != 0) return -1;
    } else if (stop_rd) {
        const size_t sm = sizeof(qtts_samp::KSmem);
        if (a.n <= 8 * 256) {
            hipLaunchKernelGGL((k_sample_pg<8>), dim3(a.nb), dim3(256), sm, st, stop_rd, a, tab);
            qtts_last_kernel = "k_sample_pg<8>";
        } else {
            hipLaunchKernelGGL((k_sample_pg<qtts_samp::EMAX>), dim3(a.nb), dim3(256), sm, st, stop_rd, a, tab);
            qtts_last_kernel = "k_sample_pg<16>";
        }
    } else {
        const size_t sm = sizeof(qtts_samp::KSmem);
        if (a.n <= 8 * 256) {
            hipLaunchKernelGGL((k_sample_p<8>), dim3(a.nb), dim3(256), sm, st, a, tab);
            qtts_last_kernel = "k_sample_p<8>";
        } else {
            hipLaunchKernelGGL((k_sample_p<qtts_samp::EMAX>), dim3(a.nb), dim3(256), sm, st, a, tab);
            qtts_last_kernel = "k_sample_p<16>";
        }
    }
    if (hipGetLastError() != hipSuccess) return -1;
    g_slot_launches.fetch_add(1);
    return 0;
}
