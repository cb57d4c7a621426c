// k_sample_f.hip - the sampler's forced form (teacher forcing, the free-draw
// record and logit taps; qtts_kernels.h SampForce, the device code in
// qtts_sample_dev.h sample_row<..., FORCE>): one instantiation beside each
// plain kernel of k_sample.hip.  A file of its own so that k_sample.hip's
// object -- the plain kernels every unarmed run launches -- stays instruction
// for instruction what it was.
#include "qtts_sample_dev.h"

namespace {

// the forced forms (teacher forcing and taps, qtts_kernels.h SampForce): the
// plain kernels' arguments first and unchanged, the extra pointers after them
template <bool FAST, int EM>
__global__ __launch_bounds__(256) void k_sample_f(SampArgs a, SampForce f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row<FAST, EM, 256, true>(a, blockIdx.x, smraw, a.logits, a.stopped,
                                               a.mode == 1 ? a.rng : a.st_rng, a.n_gen, a.counts, &f);
}

template <int EM>
__global__ __launch_bounds__(1024) void k_sample_wf(const float *logits, const int *stopped, const uint32_t *rng,
                                                    const int *n_gen, const int *counts, SampArgs a, SampForce f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    qtts_samp::sample_row<true, EM, 1024, true>(a, blockIdx.x, smraw, logits, stopped, rng, n_gen, counts, &f);
}

}  // namespace

// the same choice of launch family as qtts_sample, on the forced kernels
int qtts_sample_forced(const SampArgs &a, const SampForce &f, hipStream_t st) {
#ifdef QTTS_ARGDUMP
    qtts_argdump::samp("qtts_sample_forced", a, 0, nullptr, nullptr, &f);
#endif
    if (a.n > qtts_samp::NMAX || a.n < 1) {
        fprintf(stderr, "qtts_sample: vocab %d unsupported (max %d)\n", a.n, qtts_samp::NMAX);
        return -1;
    }
    if (!f.forced || !f.drawn || !f.taps || !f.tap_logits || !f.tap_meta || f.tap_ld < a.n || !a.codes || !a.cur_row) {
        fprintf(stderr, "qtts_sample_forced: incomplete arguments\n");
        return -1;
    }
    const char *sw = getenv("QTTS_HIP_SAMPLE_W");
    if (qtts_samp::fast_path(a) && !(sw && !atoi(sw))) {
        const size_t sm = sizeof(qtts_samp::FastSmemNT<1024>);
        const uint32_t *rng = a.mode == 1 ? a.rng : a.st_rng;
        if (a.n <= 2 * 1024) {
            hipLaunchKernelGGL((k_sample_wf<2>), dim3(a.nb), dim3(1024), sm, st, a.logits, (const int *)a.stopped, rng,
                               (const int *)a.n_gen, (const int *)a.counts, a, f);
            qtts_last_kernel = "k_sample_wf<2>";
        } else {
            hipLaunchKernelGGL((k_sample_wf<4>), dim3(a.nb), dim3(1024), sm, st, a.logits, (const int *)a.stopped, rng,
                               (const int *)a.n_gen, (const int *)a.counts, a, f);
            qtts_last_kernel = "k_sample_wf<4>";
        }
    } else if (qtts_samp::fast_path(a)) {
        const size_t sm = sizeof(qtts_samp::FastSmem);
        if (a.n <= 8 * 256) {
            hipLaunchKernelGGL((k_sample_f<true, 8>), dim3(a.nb), dim3(256), sm, st, a, f);
            qtts_last_kernel = "k_sample_f<true, 8>";
        } else {
            hipLaunchKernelGGL((k_sample_f<true, 16>), dim3(a.nb), dim3(256), sm, st, a, f);
            qtts_last_kernel = "k_sample_f<true, 16>";
        }
    } else {
        hipLaunchKernelGGL((k_sample_f<false, qtts_samp::EMAX>), dim3(a.nb), dim3(256), sizeof(qtts_samp::KSmem), st, a,
                           f);
        qtts_last_kernel = "k_sample_f<false, 16>";
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
