// k_sample_n.hip - the sampler with the nucleus short list (qtts_sample_dev.h
// sample_nucleus, sample_row_n): top_p < 1 with top_k <= 64 or top-k off draws
// from at most 64 ids and one sequential sum over the vocabulary instead of
// the full path's two sorts and five one-lane loops, and falls back to the
// full path inside the same launch when the short list cannot decide.  A file
// of its own, as k_sample_f.hip and k_sample_p.hip are, so that their objects
// and k_sample.hip's -- the kernels every default run launches -- stay what
// they were.
//
//   k_sample_n<false, EM>  the parameters of SampArgs (k_sample<false, EM>'s place)
//   k_sample_n<true, EM>   row b of the per-slot table (k_sample_p<EM>'s place):
//                          fast, nucleus-short or full per row, a
//                          workgroup-uniform branch
// 256 threads on the general kernel's LDS, which the in-launch fallback needs.
// stop_rd (a fed run's gate, may be NULL: a.stopped), path (may be NULL: the
// path each row took, see sample_row_n) and the nucleus switch are arguments
// of their own outside SampArgs, so no other kernel's argument layout moves.
#include "qtts_sample_dev.h"

namespace {

template <bool SLOT, int EM>
__global__ __launch_bounds__(256) void k_sample_n(const int *stop_rd, SampArgs a, const SampSlotRow *tab, int *path,
                                                  int nucleus) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row_n<SLOT, EM>(a, tab, blockIdx.x, smraw, stop_rd ? stop_rd : a.stopped, path, nucleus != 0);
}

bool args_ok(const SampArgs &a) {
    if (a.n > qtts_samp::NMAX || a.n < 1) {
        fprintf(stderr, "qtts_sample: vocab %d unsupported (max %d)\n", a.n, qtts_samp::NMAX);
        return false;
    }
    return true;
}

}  // namespace

bool qtts_sample_nucleus_on() {
    const char *s = getenv("QTTS_HIP_SAMPLE_NUCLEUS");
    return !(s && !atoi(s));
}

bool qtts_sample_nucleus_row(float top_p, int top_k, int n) { return qtts_samp::nucleus_row(top_p, top_k, n); }

int qtts_sample_n(const SampArgs &a, hipStream_t st, const int *stop_rd, int *path, bool nucleus) {
    if (!args_ok(a)) return -1;
    const size_t sm = sizeof(qtts_samp::NKSmem);
    if (a.n <= 8 * 256) {
        hipLaunchKernelGGL((k_sample_n<false, 8>), dim3(a.nb), dim3(256), sm, st, stop_rd, a,
                           (const SampSlotRow *)nullptr, path, (int)nucleus);
        qtts_last_kernel = "k_sample_n<false, 8>";
    } else {
        hipLaunchKernelGGL((k_sample_n<false, qtts_samp::EMAX>), dim3(a.nb), dim3(256), sm, st, stop_rd, a,
                           (const SampSlotRow *)nullptr, path, (int)nucleus);
        qtts_last_kernel = "k_sample_n<false, 16>";
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int qtts_sample_slots_n(const SampArgs &a, const SampSlotRow *tab, hipStream_t st, const int *stop_rd, int *path,
                        bool nucleus) {
    if (!args_ok(a)) return -1;
    if (!tab) {
        fprintf(stderr, "qtts_sample_slots: no parameter table\n");
        return -1;
    }
    const size_t sm = sizeof(qtts_samp::NKSmem);
    if (a.n <= 8 * 256) {
        hipLaunchKernelGGL((k_sample_n<true, 8>), dim3(a.nb), dim3(256), sm, st, stop_rd, a, tab, path, (int)nucleus);
        qtts_last_kernel = "k_sample_n<true, 8>";
    } else {
        hipLaunchKernelGGL((k_sample_n<true, qtts_samp::EMAX>), dim3(a.nb), dim3(256), sm, st, stop_rd, a, tab, path,
                           (int)nucleus);
        qtts_last_kernel = "k_sample_n<true, 16>";
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
