// pdegym_backstep_law.h -- the dot product of the backstepping control law, a = (sum_{i<len} gain[i] * (double)obs[i]) * scale, in its two
// orders of addition (include/pdegym.h: PDEGYM_BACKSTEP_TREE / _ORDERED).  ONE copy, shared by the control kernel (pdegym_backstep.hip:
// operands from memory) and the one-launch rollout kernel (pdegym_backstep_rollout.hip: gains in registers, the row in LDS), so that the
// two paths cannot drift apart: they are bit-identical because they ARE the same additions.
#ifndef PDEGYM_BACKSTEP_LAW_H
#define PDEGYM_BACKSTEP_LAW_H

#include <hip/hip_runtime.h>

#include "pdegym_common.h"

namespace pdegym_backstep_law {

using namespace pdegym::wave;      // kWave, lane_value, wave_sum

// s + p[0] + p[1] + ... + p[cnt - 1] over the lanes of `p`, added one after the other in that order (cnt wave-uniform, <= 64):
// the left-to-right chain of a Python loop / the builtin sum.  Result in every lane.
__device__ __forceinline__ double chain_add(double s, double p, int cnt) {
  for (int l = 0; l < cnt; ++l) s += lane_value(p, l);
  return s;
}

// sum_{i<len} term(k, i) over chunks k of 64 terms, lane l of chunk k forming term i = 64 k + l (term: the product of that index, double):
//   ORDERED  chain_add over the chunks in turn: i ascending from 0.0;
//   TREE     lane l adds i = l, l + 64, ... in ascending order, then the wave reduction.
// NK == 0: as many chunks as len needs (a run-time loop); NK > 0: at most NK chunks, len <= 64 NK, the loop unrolled so that a caller may
// keep per-chunk operands in registers (term's k is then a compile-time constant).  Result in every lane.
template <bool ORDERED, int NK = 0, typename Term>
__device__ __forceinline__ double dot(int len, int lane, Term&& term) {
  double s = 0.0;
  auto chunk = [&](int k, int base) {
    const int i = base + lane;
    if constexpr (ORDERED) {
      const double p = i < len ? term(k, i) : 0.0;
      s = chain_add(s, p, min(kWave, len - base));
    } else {
      if (i < len) s += term(k, i);
    }
  };
  if constexpr (NK > 0) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k * kWave < len) chunk(k, k * kWave);      // wave-uniform
  } else if constexpr (ORDERED) {
    int k = 0;
    for (int base = 0; base < len; base += kWave, ++k) chunk(k, base);
  } else {
    int k = 0;
    for (int i = lane; i < len; i += kWave, ++k) s += term(k, i);
  }
  return ORDERED ? s : wave_sum(s);
}

}  // namespace pdegym_backstep_law
#endif
