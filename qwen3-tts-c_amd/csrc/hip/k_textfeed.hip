// k_textfeed.hip - incremental text input (DESIGN.md "Incremental text input").
//
// The append: up to QTTS_TF_MAX content ids of one slot go through
// text_embedding -> fc1 (+bias, SiLU) -> fc2 (+bias) into the slot's trailing
// rows, behind the rows already there (the offset is n_trailing[b], read on the
// device), and a last one-block launch publishes the new count.  The ids travel
// as kernel arguments, so the call makes no copy and no host wait.
//
// One kernel path for every id: a wave owns one output row and keeps one
// accumulator per appended id; lane l adds columns l, l + 64, ... in that order
// and the 64 lane sums are folded by the same xor butterfly.  A row's value
// therefore does not depend on how many ids share its launch (the rows of
// qtts_dev_prompt change kernel with their count: k_gemv / k_gemvb / k_mgemm).
//
// The hold: a fed run's frame graphs start with k_text_gate,
//   gate[b] = stopped[b] | (text_open[b] && n_gen[b] >= n_trailing[b]),
// (the frame that draws frame r adds trailing row r: the sampler sets
// cur_row = n_gen, k_embed_sum reads trailing[cur_row]) and every reader of the
// stop flag takes `gate` instead.  A held slot's talker input row is saved by
// the same launch and put back by k_text_restore at the frame's end: the talker
// layers update the residual in place.  Nothing waits on a flag: a starved slot
// is skipped for the frame and looked at again by the next launch.
#include "qtts_common.h"
#include "qtts_kernels.h"

namespace {

template <int STAGE>
__global__ __launch_bounds__(256) void k_tf_proj(TextFeedArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.TH, R = STAGE == 0 ? a.TH : a.H;
    const int r = blockIdx.x * 4 + wave;
    if (r >= R) return;   // (wave-uniform; no barrier below)
    const bf16_t *W = (STAGE == 0 ? a.fc1w : a.fc2w) + (size_t)r * C;
    const int n = a.n;
    float acc[QTTS_TF_MAX];
#pragma unroll
    for (int j = 0; j < QTTS_TF_MAX; ++j) acc[j] = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float w = bf2f(W[c]);
#pragma unroll
        for (int j = 0; j < QTTS_TF_MAX; ++j) {
            if (j < n) {   // (uniform)
                const float x = STAGE == 0 ? bf2f(a.text_emb[(size_t)a.ids[j] * C + c]) : a.t1[(size_t)j * C + c];
                acc[j] = fmaf(w, x, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QTTS_TF_MAX; ++j)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
    if (lane != 0) return;
    if (STAGE == 0) {
        const float bias = a.fc1b[r];
#pragma unroll
        for (int j = 0; j < QTTS_TF_MAX; ++j) {
            if (j < n) {
                const float z = acc[j] + bias;
                a.t1[(size_t)j * C + r] = z / (1.0f + expf(-z));
            }
        }
    } else {
        const float bias = a.fc2b ? a.fc2b[r] : 0.0f;
        const int base = a.n_trailing[a.b];
#pragma unroll
        for (int j = 0; j < QTTS_TF_MAX; ++j) {
            if (j < n && base + j < a.tr_cap)   // (the host grows the rows first; never past the slot's block)
                a.trailing[((size_t)a.b * a.tr_cap + base + j) * a.H + r] = acc[j] + bias;
        }
    }
}

// the tts_eos row of a close, then the new count: the append's last store
__global__ __launch_bounds__(256) void k_tf_publish(TextFeedArgs a) {
    const int base = a.n_trailing[a.b];
    int rows = base + a.n;
    if (a.close && rows < a.tr_cap) {
        float *dst = a.trailing + ((size_t)a.b * a.tr_cap + rows) * a.H;
        for (int d = threadIdx.x; d < a.H; d += 256) dst[d] = a.eos[d];
        rows += 1;
    }
    if (rows > a.tr_cap) rows = a.tr_cap;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        if (a.close) a.text_open[a.b] = 0;
        a.n_trailing[a.b] = rows;
    }
}

__global__ __launch_bounds__(256) void k_text_gate(TextGateArgs a) {
    const int b = blockIdx.y;
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (a.x_save && d < a.H) a.x_save[(size_t)b * a.H + d] = a.x[(size_t)b * a.H + d];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int stop = a.stopped[b];
        const int starved = a.text_open[b] && a.n_gen[b] >= a.n_trailing[b];
        a.gate[b] = stop | starved;
        if (!stop && starved) a.held[b] += 1;
    }
}

__global__ __launch_bounds__(256) void k_text_restore(TextGateArgs a) {
    const int b = blockIdx.y;
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (a.gate[b] && d < a.H) a.x[(size_t)b * a.H + d] = a.x_save[(size_t)b * a.H + d];
}

// slot b's text opens: its only trailing row (tts_eos, as qtts_dev_prompt
// projected it) moves to the slot's eos row and the count goes back to 0
__global__ __launch_bounds__(256) void k_text_open(float *eos, const float *trailing_row, int H, int *n_trailing,
                                                   int *text_open, int *held, int b) {
    for (int d = threadIdx.x; d < H; d += 256) eos[d] = trailing_row[d];
    if (threadIdx.x == 0) {
        n_trailing[b] = 0;
        text_open[b] = 1;
        held[b] = 0;
    }
}

}  // namespace

int qtts_text_append(const TextFeedArgs &a, hipStream_t st) {
    if (a.n < 0 || a.n > QTTS_TF_MAX || (a.n == 0 && !a.close)) return -1;
    if (a.n > 0) {
        hipLaunchKernelGGL((k_tf_proj<0>), dim3((a.TH + 3) / 4), dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_tf_proj<1>), dim3((a.H + 3) / 4), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_tf_publish, dim3(1), dim3(256), 0, st, a);
    qtts_last_kernel = "k_tf_publish";
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int qtts_text_gate(const TextGateArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_text_gate, dim3((a.H + 255) / 256, a.nb), dim3(256), 0, st, a);
    qtts_last_kernel = "k_text_gate";
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int qtts_text_restore(const TextGateArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_text_restore, dim3((a.H + 255) / 256, a.nb), dim3(256), 0, st, a);
    qtts_last_kernel = "k_text_restore";
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int qtts_text_open(float *eos, const float *trailing_row, int H, int *n_trailing, int *text_open, int *held, int b,
                   hipStream_t st) {
    hipLaunchKernelGGL(k_text_open, dim3(1), dim3(256), 0, st, eos, trailing_row, H, n_trailing, text_open, held, b);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
