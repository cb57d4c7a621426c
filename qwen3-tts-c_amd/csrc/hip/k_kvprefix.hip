// k_kvprefix.hip - save / restore of a cached talker KV prefix (the instruct
// rows of a prompt, DESIGN.md "Instruct and the prefix cache").
#include "qtts_common.h"
#include "qtts_kernels.h"

namespace {

// blockIdx.y = which * L + l: one layer's rows [0, n) of K (which 0) or V (1),
// `chunk` contiguous bytes on both sides.  16-byte accesses over the part both
// sides have 16-byte aligned, element-sized ones for the tail (or for all of
// it where a base is not aligned: a row of KV*HD elements that is no multiple
// of 16 bytes).  A plain copy: what is restored is bit for bit what was saved.
__global__ __launch_bounds__(256) void k_kv_prefix(KvPrefixArgs a) {
    const int which = (int)blockIdx.y / a.L, l = (int)blockIdx.y % a.L;
    char *cache = reinterpret_cast<char *>(which ? a.vc : a.kc) + (size_t)l * a.layer_stride;
    char *entry = reinterpret_cast<char *>(a.entry) + (size_t)blockIdx.y * a.chunk;
    const char *src = a.save ? cache : entry;
    char *dst = a.save ? entry : cache;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    const size_t nvec = aligned ? a.chunk / 16 : 0;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (size_t i = tid; i < nvec; i += nth) d4[i] = s4[i];
    const size_t done = nvec * 16;
    if (a.esz == 4) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src + done);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst + done);
        for (size_t i = tid; i < (a.chunk - done) / 4; i += nth) d[i] = s[i];
    } else {
        const uint16_t *s = reinterpret_cast<const uint16_t *>(src + done);
        uint16_t *d = reinterpret_cast<uint16_t *>(dst + done);
        for (size_t i = tid; i < (a.chunk - done) / 2; i += nth) d[i] = s[i];
    }
}

}  // namespace

int qtts_kv_prefix_copy(const KvPrefixArgs &a, hipStream_t st) {
    if (!a.kc || !a.vc || !a.entry || a.L < 1 || a.chunk == 0 || (a.esz != 2 && a.esz != 4) || a.chunk % a.esz)
        return -1;
    size_t bx = (a.chunk / 16 + 255) / 256;
    if (bx < 1) bx = 1;
    if (bx > 128) bx = 128;
    hipLaunchKernelGGL(k_kv_prefix, dim3((unsigned)bx, (unsigned)(2 * a.L)), dim3(256), 0, st, a);
    qtts_last_kernel = "k_kv_prefix";
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
