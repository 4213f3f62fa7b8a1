// many_common.h -- what the MFMA passes over a half gallery share (search_many.hip: the nearest `depth`; range_many.hip: every row within a
// radius): the query prologue, the layout of the B-fragment image it writes, the A-fragment loader of a tile of 16 stored rows, and the
// constant of the error bound that search_many.hip derives.  One copy, so that the two passes cannot drift: both multiply the same
// operands and bound the same approximate distance A.
#pragma once
#include "search_walk.h"

namespace {
using namespace vtcsweep;

constexpr int MANY_MAX_Q = 64;         // queries of a call at most: four waves of 16
constexpr int MANY_KC = 512;           // columns of a K chunk: 16 MFMA steps, 32 KB of B fragments a wave
constexpr int MANY_KS = MANY_KC / 32;
constexpr int QF_DEAD = 1, QF_FALLBACK = 2;

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

// |A - D| <= many_kappa(d) (|q|^2 + |g|^2) + 1e-35 for every pair whose A is finite and whose query is not QF_FALLBACK (search_many.hip)
inline float many_kappa(int d) { return (6.0f * d + 8.0f) / 16777216.0f + 1.0f / 1048576.0f; }
inline int many_qgroups(int nq) { return cdiv(nq, 16); }
// The B-fragment image of the queries: uint4 [qgroups][d / 32][hi, lo][64 lanes].  The fragment of MFMA step ks: lane (kq, u) = 16 kq + u
// holds the 8 halves k = 32 ks + 8 kq .. + 7 of query u of the group.
inline size_t many_img_bytes(int nq, int d) { return (size_t)many_qgroups(nq) * 16 * d * 2 * sizeof(_Float16); }
__device__ __forceinline__ size_t many_img_at(int grp, int d, int ks, int kq, int u) {      // of the hi fragment; lo is 64 further
  return ((size_t)(grp * (d / 32) + ks) * 2) * 64 + kq * 16 + u;
}
// MFMA steps of an item of a pass: the largest of 16, 8, 4, 2 that divides the row's d / 32 (d % 64 == 0: that is even)
inline int many_item_steps(int d) {
  const int ksteps = d / 32;
  return ksteps % 16 == 0 ? 16 : (ksteps % 8 == 0 ? 8 : (ksteps % 4 == 0 ? 4 : 2));
}

// One wave per query slot (16 x qgroups of them; a slot past the last query is a dead row of zeros, as a query with a NaN / inf is).
// Zeroes the call's counter, `counter_words` int32 of it.
__global__ __launch_bounds__(64) void many_prep_kernel(const float *__restrict__ queries, int nq, int d, uint4 *__restrict__ qimg,
                                                       float *__restrict__ qn, float *__restrict__ inv_s, int *__restrict__ qflag,
                                                       int *__restrict__ counter, int counter_words, int *__restrict__ nonfinite) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q == 0 && lane < counter_words) counter[lane] = 0;
  const float *row = queries + (size_t)min(q, nq - 1) * d;
  float m = 0.f, n2 = 0.f;
  bool bad = false;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4 *>(row + c);
    bad = bad || !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    n2 = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, n2))));
  }
  const bool nonfin = __ballot(bad) != 0, dead = nonfin || q >= nq;
  m = wave_max(dead ? 0.f : m);
  n2 = wave_sum(n2);
  int flag = dead ? QF_DEAD : 0, e = 13;                   // m == 0: s = 1
  if (m > 0.f) e = ilogbf(m);
  int se = 13 - e;                                         // s = 2^se puts m into [2^13, 2^14)
  if (se > 126) {                                          // a query below 2^-113: s would leave fp32, the split has no bound
    se = 126;
    flag |= QF_FALLBACK;
  }
  const float s = __int_as_float((se + 127) << 23);
  if (lane == 0) {
    qn[q] = dead ? 0.f : n2;
    inv_s[q] = __int_as_float((127 - se) << 23);
    qflag[q] = flag;
    if (nonfin && q < nq && nonfinite) atomicOr(nonfinite, 2);
  }
  const int grp = q >> 4, u = q & 15;
  for (int b = lane; b < d / 8; b += 64) {
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = dead ? 0.f : row[b * 8 + j] * s;
      hi[j] = (_Float16)x;
      lo[j] = (_Float16)(x - (float)hi[j]);
    }
    const size_t o = many_img_at(grp, d, b >> 2, b & 3, u);
    qimg[o] = __builtin_bit_cast(uint4, hi);
    qimg[o + 64] = __builtin_bit_cast(uint4, lo);
  }
}

// The A fragments of an item -- NKS MFMA steps of tile t, the 16 rows 16 t .. 16 t + 15: lane (kq, u) holds row u of the tile, halves
// 32 ks + 8 kq .. + 7 of chunk `chunk`, 16 bytes straight from global memory.  `bits`: the tile's rows that are live and inside the
// gallery, != 0.  A dead row (or one past the gallery) is pointed at a live row of the tile: its memory is not read, its results are
// dropped by the caller.
template <int NKS>
__device__ __forceinline__ void many_load_frags(const _Float16 *gallery, int d, long long t, int chunk, unsigned bits, int u, int kq,
                                                f16x8 (&ga)[NKS]) {
  const long long row = t * 16 + (((bits >> u) & 1) ? u : __ffs((int)bits) - 1);
  const _Float16 *p = gallery + (size_t)row * d + chunk * (NKS * 32) + kq * 8;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) ga[ks] = *reinterpret_cast<const f16x8 *>(p + ks * 32);
}
}  // namespace
