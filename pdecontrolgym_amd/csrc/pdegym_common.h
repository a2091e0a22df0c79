// pdegym_common.h -- error slot and launch check shared by the C-ABI translation units, and (second half) the wave64 device
// primitives shared by their kernels: lane shifts, wave reductions, wait counts, the reset-pool row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pdegym {

// thread-local message returned by pdegym_last_error(); defined in pdegym_abi.hip
char* error_slot();
int fail(int code, const char* msg);
int check_launch(const char* what);

// Pointers need only the natural alignment of their element type (include/pdegym.h, Conventions).  Where a parameter states more --
// its kernel reads it through a naturally aligned 16-byte type -- the host function refuses another pointer before it launches.
inline bool is_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// Per-device caches: the library keeps no state that is bound to "the first device that called" (a process may drive
// several GPUs, one engine per device, each call made with that engine's device current).
constexpr int kMaxDevices = 64;
// The thread's current device and its cache slot: devices beyond kMaxDevices have no slot (-1) and are queried every time --
// they are never mistaken for device 0.
inline int current_device(int* slot = nullptr) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if (slot) *slot = dev < kMaxDevices ? dev : -1;
  return dev;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel call site, device); `slots` is that site's static array
inline bool raise_dynamic_lds_limit(const void* kernel, int bytes, signed char (&slots)[kMaxDevices]) {
  int slot;
  current_device(&slot);
  if (slot < 0) return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  if (slots[slot] == 0)
    slots[slot] = (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) ? 1 : -1;
  return slots[slot] > 0;
}

// SIMDs of the current device (compute units x 4), cached per device: launch heuristics that mean "at most one wave per SIMD" ask
// here instead of assuming the 256 CUs of an unpartitioned MI355X (a CPX / DPX partition or another SKU has fewer).
inline int simd_count() {
  static int cached[kMaxDevices] = {};
  int slot;
  const int dev = current_device(&slot);
  if (slot >= 0 && cached[slot] != 0) return cached[slot];
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  if (slot >= 0) cached[slot] = cus * 4;
  return cus * 4;
}

// ---- device side ------------------------------------------------------------------------------------------------------------------
// min(max(x, lo), hi) as the reference's clamps evaluate it (np.clip, torch.clamp, Python's min(max(x, lo), hi) with x first): a NaN x
// stays NaN -- the device's fmin / fmax return the operand that is NOT NaN, which would turn a diverged command into the lower bound.
// Every other x keeps the bits the plain form gives (signed zeros and infinities included).  The bounds are finite by contract.
__device__ __forceinline__ float clip_keep_nan(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ double clip_keep_nan(double x, double lo, double hi) { return x != x ? x : fmin(fmax(x, lo), hi); }

// the wave64 primitives of every kernel family
namespace wave {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;      // one instance per wave, four waves per workgroup (the policy kernels: pdegym_policy::kWaves)

// LDS written by some lanes of a wave is visible to all of them (wave-level ordering only: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// s_waitcnt vmcnt(0) as a real instruction (the compiler's wait-count pass sees it): the carried rollout loops end every RARE
// path that loads (exact redo, auto-reset, a batch of commands handed over) with it, so that no register is "possibly still being
// loaded" at the loop's back edge -- otherwise the pass puts a static vmcnt(0) in front of the first use of each such register in
// EVERY iteration, and on gfx9 that also waits for all the stores in flight (vmcnt counts both).
__device__ __forceinline__ void drain_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // vmcnt(0), expcnt / lgkmcnt untouched

// One DPP move (v_mov_b32_dpp): CTRL is the control word, ROW_MASK the rows of 16 lanes that are written; a lane without a source
// or in a masked row gets `old` (BOUND_CTRL: a lane without a source gets 0 instead).  double: the two halves move separately.
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp_move(float v, float old = 0.f) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK,
                                                               0xf, BOUND_CTRL));
}
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ double dpp_move(double v, double old = 0.0) {
  const long long b = __builtin_bit_cast(long long, v), o = __builtin_bit_cast(long long, old);
  const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, CTRL, ROW_MASK, 0xf, BOUND_CTRL);
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), CTRL, ROW_MASK, 0xf, BOUND_CTRL);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// lane i <- lane i-1 ; lane 0 <- `edge`      (DPP wave_shr:1, gfx9 wave-wide shift)
__device__ __forceinline__ float from_left_lane(float v, float edge) { return dpp_move<0x138>(v, edge); }
// lane i <- lane i+1 ; lane 63 <- `edge`     (DPP wave_shl:1)
__device__ __forceinline__ float from_right_lane(float v, float edge) { return dpp_move<0x130>(v, edge); }
// the same shifts where the lane without a source gets 0 (never used: it is a domain-edge thread)
template <typename T>
__device__ __forceinline__ T lane_left(T v) { return dpp_move<0x138, 0xf, true>(v); }
template <typename T>
__device__ __forceinline__ T lane_right(T v) { return dpp_move<0x130, 0xf, true>(v); }
// A lane shift must execute with every lane of the wave active: when its only use is a per-lane select or sits in a branch that
// masks lanes off (edge lanes keep their value, an inner update runs on lanes 1 .. M-2 only), the compiler may fold the shift into
// that branch, and a DPP read from a lane that is masked off returns 0.  The empty asm pins the shift where it is written.
// (ds_bpermute -- __shfl_up / __shfl_down -- costs an LDS round trip per shuffle.)
template <typename T>
__device__ __forceinline__ T pinned_from_left(T v) {
  T r = lane_left(v);
  asm volatile("" : "+v"(r));
  return r;
}
template <typename T>
__device__ __forceinline__ T pinned_from_right(T v) {
  T r = lane_right(v);
  asm volatile("" : "+v"(r));
  return r;
}

// value of lane l (wave-uniform) in every lane
__device__ __forceinline__ float lane_value(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double lane_value(double v, int l) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// Wave-wide reductions on DPP (result in every lane).  __shfl_xor compiles to ds_bpermute_b32, an LDS round trip per step (two per
// double): six dependent ones per reduction, each ~25 cycles of the wave's SIMD (docs/HISTORY.md section 4: tools/attic/ab_ns_col.py),
// on the critical path of a wave's prologue / epilogue.
// Steps: the lane pair, the quad (quad_perm), the half row and the row (row_half_mirror / row_mirror: lane i pairs with
// lane 7-i / 15-i), then lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15) and lane 31 into rows 2, 3
// (row_bcast:31): lane 63 holds the total, v_readlane hands it to everybody.  A fixed order (deterministic), not the
// butterfly's -- norms and rewards were never bitwise against a BLAS dot product anyway (tests: rtol 1e-6 in float, 1e-12 in
// double); every kernel of a family shares it, so step and rollout kernels stay bit-identical to each other.
// Lanes without a source (the masked rows of the last two steps) read 0: sums, and maxima of magnitudes.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  v = op(v, dpp_move<0xB1>(v));          // quad_perm:[1,0,3,2]
  v = op(v, dpp_move<0x4E>(v));          // quad_perm:[2,3,0,1]
  v = op(v, dpp_move<0x141>(v));         // row_half_mirror
  v = op(v, dpp_move<0x140>(v));         // row_mirror
  v = op(v, dpp_move<0x142, 0xa>(v));    // row_bcast:15 -> rows 1, 3
  v = op(v, dpp_move<0x143, 0xc>(v));    // row_bcast:31 -> rows 2, 3
  return lane_value(v, 63);
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  return wave_reduce(v, [](T a, T b) { return a + b; });
}

// Row of the reset pools that restart number count[inst] + extra of instance `inst` takes, (inst + k*B) mod rows (include/pdegym.h:
// reset_pool_rows, 0 = B; count NULL = always row inst).  extra: restarts made inside the launch and not yet added to count.
// Returned as the 64-bit remainder it is: callers index with it or narrow it themselves.
__device__ __forceinline__ long long pool_row(int rows, const int32_t* count, int inst, int B, int extra = 0) {
  rows = rows > 0 ? rows : B;
  const long long k = (count ? (long long)count[inst] : 0) + extra;
  return ((long long)inst + k * (long long)B) % rows;
}

}  // namespace wave
}  // namespace pdegym
