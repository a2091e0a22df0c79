// lds_residue.hip -- test-only: leave a known bit pattern in every CU's LDS, and read LDS back without writing it.
//
// LDS is not cleared between launches: a workgroup starts on what the previous kernel on its CU left there.  The suite's GPU tests
// launch the same kernels on similar data over and over, so that residue is always finite, plausible floats; these two kernels make
// it a pattern of the test's choosing (tests/lds_residue.py, tests/test_gpu_lds_residue.py).
//
//   lds_dirty   : groups_per_cu x (CU count) workgroups of 256 threads, each with the LARGEST dynamic LDS segment the device grants
//                 one workgroup (the CU's whole LDS where the runtime allows it, so that one workgroup owns one CU's LDS), fill it
//                 with a 64-bit pattern: low word at even dword index, high word at odd.  Lane 0 stores 1 to seen[__smid()].
//   lds_witness : a grid and a segment size of the caller's choosing; reads the segment it never wrote and reports, per thread, how
//                 many dwords hold the pattern, and per workgroup its __smid().
//   lds_pad_probe : the defect the suite looks for, in a kernel of its own (the product has none to show): one wave stages a row of
//                 n floats "zero-padded to a multiple of four" and reduces the padded row -- with the pad written, or left as found.
//
// Plain C++ with vector (per-lane) stores only.  Built into pdecontrolgym_amd/lib/libpdegym_lds_residue.so by
// pdecontrolgym_amd/build.py (build_lds_residue), on demand from tests/lds_residue.py; NOT part of the product ABI and not under csrc/, so no kernel fingerprint depends on it.
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void lds_dirty_kernel(uint32_t lo, uint32_t hi, int words, int32_t* seen, int seen_cap) {
    extern __shared__ __attribute__((aligned(16))) uint32_t seg[];
    volatile uint32_t* s = seg;              // (volatile: these stores have no reader in this kernel and must still happen)
    for (int i = threadIdx.x; i < words; i += kBlock) s[i] = (i & 1) ? hi : lo;
    if (threadIdx.x == 0 && seen) {
        const unsigned id = __smid();
        if (id < (unsigned)seen_cap) seen[id] = 1;
    }
}

__global__ __launch_bounds__(kBlock) void lds_witness_kernel(uint32_t lo, uint32_t hi, int words, int32_t* partial, int32_t* smid) {
    extern __shared__ __attribute__((aligned(16))) uint32_t seg[];
    const volatile uint32_t* s = seg;
    int hit = 0;
    for (int i = threadIdx.x; i < words; i += kBlock) hit += s[i] == ((i & 1) ? hi : lo);
    partial[(size_t)blockIdx.x * kBlock + threadIdx.x] = hit;
    if (threadIdx.x == 0) smid[blockIdx.x] = (int32_t)__smid();
}

// out[0] = sum_j row[j] * w[j] with w = 1 below n and 0 in the pad (a product with a zero weight: 0 * residue); out[1] = sum_j row[j]
__global__ __launch_bounds__(64) void lds_pad_probe_kernel(const float* x, int n, int write_pad, float* out) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    const int lane = threadIdx.x, np = (n + 3) & ~3;
    for (int j = lane; j < n; j += 64) row[j] = x[j];
    if (write_pad)
        for (int j = n + lane; j < np; j += 64) row[j] = 0.f;
    __syncthreads();
    if (lane == 0) {
        const volatile float* r = row;
        float dot = 0.f, sum = 0.f;
        for (int j = 0; j < np; ++j) {
            const float v = r[j];
            dot = __builtin_fmaf(v, j < n ? 1.f : 0.f, dot);
            sum += v;
        }
        out[0] = dot;
        out[1] = sum;
    }
}

namespace {
struct Info {
    int ready = 0, cus = 0, max_bytes = 0;
};
Info g_info[64];

// CU count and the largest dynamic segment lds_dirty_kernel may have on the current device (found once per device, outside of any
// stream capture: the first call comes from dirtied().__enter__ or from a test, before anything is enqueued)
const Info* info() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    Info& I = g_info[dev];
    if (I.ready) return &I;
    int cus = 0, per_cu = 0, per_wg = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return nullptr;
    if (hipDeviceGetAttribute(&per_wg, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return nullptr;
    if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess) per_cu = 0;
    // the CU's whole LDS if the runtime grants it to one workgroup, else the per-workgroup figure it reports
    int bytes = 0;
    if (per_cu > per_wg && hipFuncSetAttribute((const void*)lds_dirty_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, per_cu) == hipSuccess &&
        hipFuncSetAttribute((const void*)lds_witness_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, per_cu) == hipSuccess)
        bytes = per_cu;
    else if (hipFuncSetAttribute((const void*)lds_dirty_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, per_wg) == hipSuccess &&
             hipFuncSetAttribute((const void*)lds_witness_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, per_wg) == hipSuccess)
        bytes = per_wg;
    (void)hipGetLastError();
    if (cus <= 0 || bytes < 8) return nullptr;
    I.cus = cus;
    I.max_bytes = bytes & ~7;
    I.ready = 1;
    return &I;
}
}  // namespace

// CU count and the segment size lds_dirty uses: 0, or -1
extern "C" int lds_residue_info(int32_t* cus, int32_t* max_bytes) {
    const Info* I = info();
    if (!I) return -1;
    if (cus) *cus = I->cus;
    if (max_bytes) *max_bytes = I->max_bytes;
    return 0;
}

extern "C" int lds_dirty(uint64_t pattern, int32_t* seen, int32_t seen_cap, int32_t groups_per_cu, void* stream) {
    const Info* I = info();
    if (!I || groups_per_cu <= 0 || groups_per_cu > 64 || (seen && seen_cap <= 0)) return -1;
    hipLaunchKernelGGL(lds_dirty_kernel, dim3(I->cus * groups_per_cu), dim3(kBlock), I->max_bytes, (hipStream_t)stream,
                       (uint32_t)pattern, (uint32_t)(pattern >> 32), I->max_bytes / 4, seen, seen_cap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// partial: grid * 256 int32, smid: grid int32
extern "C" int lds_witness(uint64_t pattern, int32_t lds_bytes, int32_t grid, int32_t* partial, int32_t* smid, void* stream) {
    const Info* I = info();
    if (!I || !partial || !smid || grid <= 0 || lds_bytes < 8 || lds_bytes % 8 || lds_bytes > I->max_bytes) return -1;
    hipLaunchKernelGGL(lds_witness_kernel, dim3(grid), dim3(kBlock), lds_bytes, (hipStream_t)stream, (uint32_t)pattern,
                       (uint32_t)(pattern >> 32), lds_bytes / 4, partial, smid);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// x: n floats (1 <= n <= 1024), out: 2 floats
extern "C" int lds_pad_probe(const float* x, int32_t n, int32_t write_pad, float* out, void* stream) {
    if (!x || !out || n < 1 || n > 1024) return -1;
    hipLaunchKernelGGL(lds_pad_probe_kernel, dim3(1), dim3(64), (size_t)((n + 3) & ~3) * sizeof(float), (hipStream_t)stream, x, n, write_pad, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
