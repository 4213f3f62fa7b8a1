// search_walk.h -- how the query-time kernels walk a stored gallery (search.hip's scan and mark pass, range.hip's count pass): the tile of
// queries in the LDS, the cursors of a page, the rows of a step under a row mask, and the tile shapes.  One copy, so that the three kernels
// cannot drift.  Host side, the cached question how many workgroups of a persistent grid a CU holds (resident_per_cu).
#pragma once
#include "sweep_common.h"

#include <type_traits>

namespace vtcsweep {

__device__ __forceinline__ double uniform_f64(double v) {      // a wave-uniform value -> scalar registers
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ int uniform_of(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uniform_of(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// The tile of NQ queries q0 .. q0 + NQ - 1 -> LDS (smem4, NQ x d floats), by the whole workgroup of 256.  A query with a NaN / inf, and a
// slot past the last query, becomes a row of zeros: every distance formed against the tile then has finite query terms, so it is
// non-finite exactly when the GALLERY row holds a NaN / inf.  Returns the DEAD bits, uniform for the workgroup: bit u is set when query
// q0 + u is such a row and takes no part.  A query with a NaN / inf sets bit 2 of *nonfinite (nullable).  Ends in a barrier.
template <int NQ>
__device__ __forceinline__ unsigned load_query_tile(const float *__restrict__ queries, int q0, int nq, int d, float4 *smem4,
                                                    int *__restrict__ nonfinite) {
  const int tid = threadIdx.x, d4 = d >> 2;
  unsigned bad_bits = 0;
  for (int x = tid; x < NQ * d4; x += 256) {
    const int u = x / d4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + u < nq) v = reinterpret_cast<const float4 *>(queries + (size_t)(q0 + u) * d)[x - u * d4];
    if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) bad_bits |= 1u << u;
    smem4[x] = v;
  }
  unsigned dead = 0;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int bad = __syncthreads_or((bad_bits >> u) & 1);
    if (bad || q0 + u >= nq) dead |= 1u << u;
    if (bad) {
      for (int x = tid; x < d4; x += 256) smem4[u * d4 + x] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nonfinite && blockIdx.x == 0 && tid == 0) atomicOr(nonfinite, 2);
    }
  }
  __syncthreads();
  return dead;
}

// The cursors (cd[u], cr[u]) of the tile's queries: the fp64 distance after_d[q] and the cursor row after_i[q] as a LOCAL row of the
// window [id_base, id_base + ng), clamp(after_i[q] - id_base, -1, ng) -- a cursor row in an earlier window is before every row of this
// one at an equal distance (-1), one in a later window after them (ng).  Wave-uniform, in scalar registers.  A row's key lies AFTER the
// cursor iff cv > cd[u] || (cv == cd[u] && row > cr[u]): a NaN cd[u] has nothing after it, -inf everything, +inf nothing.  NULLABLE: a
// null after_d (uniform for the grid) is the cursor -inf.
template <int NQ, bool NULLABLE>
__device__ __forceinline__ void load_cursors(const double *__restrict__ after_d, const int64_t *__restrict__ after_i, int64_t id_base, int ng,
                                             int q0, int nq, double (&cd)[NQ], int (&cr)[NQ]) {
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int q = min(q0 + u, nq - 1);                     // a slot past the last query is dead: its cursor is never asked
    if constexpr (NULLABLE) {
      if (!after_d) {
        cd[u] = -INFINITY;
        cr[u] = -1;
        continue;
      }
    }
    const long long a = after_i[q];
    cd[u] = uniform_f64(after_d[q]);
    cr[u] = uniform_of(a < id_base ? -1 : (int)min(a - id_base, (long long)ng));
  }
}

// A wave's walk over the gallery in steps of NR rows: wave gw of GW takes the steps gw, gw + GW, ... -- ascending rows, so exact ties
// keep (distance, row) order.  The loop itself stays in the kernel, written with the four pieces below:
//   const long long n_steps = ((long long)ng + NR - 1) / NR;
//   unsigned next_word = 0;
//   if constexpr (MASKED) { if (s < n_steps) next_word = live_word<NR>(live, s); }
//   for (; s < n_steps; s += GW) {
//     unsigned bits = 0;
//     if constexpr (MASKED) {
//       bits = live_bits<NR>(ng, s, next_word);
//       if (s + GW < n_steps) next_word = live_word<NR>(live, s + GW);
//       if (!bits) continue;              // no live row in this step: no gallery load
//     }
//     int jj[NR];
//     step_rows<NR, MASKED>(s, bits, ng, jj);
//     ... the distances of the rows jj[] ...   if (row_taken<NR, MASKED>(s, bits, r, ng)) ... row jj[r] is real ...
// They are functions of values on purpose.  A struct that carried the walk's state (the step, the stride, the word read ahead) compiled
// to other code: up to 26 more vector registers in the scan, and the masked one-query scans lost a resident wave (64 -> 66 registers).
//
// MASKED: only the rows whose bit of `live` is set take part.  A step's NR rows start at a multiple of NR, which divides 32: their bits
// lie in ONE word, and the step -- so the word -- is wave-uniform.  live_word: every lane reads the word's one address with an ordinary
// (vector) load, which returns in order -- requested a step AHEAD, before that step's gallery rows, it has arrived by the time they have
// and is never waited for on its own.  live_bits: bit r is set when row s * NR + r is live and inside the gallery (moved to a scalar
// register only there, where it is used).  step_rows: in a partly live step a dead slot is pointed at a live row of the same step and
// its results are dropped (row_taken is false), exactly as a slot past the gallery is without a mask (clamped to the last row): a dead
// row's memory is never read.  Without MASKED `live` is not looked at.
template <int NR>
__device__ __forceinline__ unsigned live_word(const unsigned *__restrict__ live, long long s) { return live[(s * NR) >> 5]; }
template <int NR>
__device__ __forceinline__ unsigned live_bits(int ng, long long s, unsigned word) {
  static_assert(32 % NR == 0, "a step's rows lie in one word");
  const int j0 = (int)(s * NR), left = ng - j0;          // s < n_steps: j0 < ng, left >= 1
  const unsigned inside = NR == 1 || left >= NR ? (1u << NR) - 1 : (1u << left) - 1;
  return (unsigned)uniform_of((int)((word >> (j0 & 31)) & inside));
}
template <int NR, bool MASKED>
__device__ __forceinline__ void step_rows(long long s, unsigned bits, int ng, int (&jj)[NR]) {
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if constexpr (MASKED) jj[r] = (int)(s * NR) + (NR == 1 || ((bits >> r) & 1) ? r : __ffs((int)bits) - 1);
    else jj[r] = (int)min(s * NR + r, (long long)ng - 1);
  }
}
template <int NR, bool MASKED>
__device__ __forceinline__ bool row_taken(long long s, unsigned bits, int r, int ng) { return MASKED ? (bits >> r) & 1 : s * NR + r < ng; }

// The tile shapes of a call: queries of a tile (a gallery pass each) x gallery rows of a step.  One query is bound by HBM and wants rows
// in flight; eight are bound by their fp64 arithmetic.  The half gallery keeps these shapes: 8 rows a step for its one- and two-query
// tiles were measured and lost (profiles/search_half.md).
struct TilePlan {
  int tile_q, tile_r, tiles;
};
inline TilePlan tile_plan(int nq) {
  TilePlan p;
  if (nq == 1) p.tile_q = 1, p.tile_r = 4;
  else if (nq == 2) p.tile_q = 2, p.tile_r = 4;
  else if (nq <= 4) p.tile_q = 4, p.tile_r = 2;
  else p.tile_q = 8, p.tile_r = 1;
  p.tiles = cdiv(nq, p.tile_q);
  return p;
}
// f(NQ, NR as integral constants) for the plan's tile shape
template <typename F>
auto with_tile(const TilePlan &p, F f) {
  if (p.tile_q == 1) return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 4>{});
  if (p.tile_q == 2) return f(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
  if (p.tile_q == 4) return f(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{});
}

// Resident workgroups per CU of a persistent grid's kernel: a property of the instantiation, its LDS (d / 64 = 1 .. 32) and the device --
// asked once, as num_cus() is, and kept in a table the launch site holds as a static of its own.  ask() puts the question (max_resident).
using ResidentTable = std::atomic<int>[64][32];
template <typename Ask>
int resident_per_cu(ResidentTable &table, int d, Ask ask) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::atomic<int> &slot = table[dev][d / 64 - 1];
  int per_cu = slot.load(std::memory_order_relaxed);
  if (per_cu == 0) {
    per_cu = ask();
    slot.store(per_cu, std::memory_order_relaxed);
  }
  return per_cu;
}
// workgroups of 256 threads and `lds` bytes of `kernel` a CU holds at once; `otherwise` when the runtime does not say
template <typename K>
int max_resident(K kernel, size_t lds, int otherwise) {
  int n = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, lds) == hipSuccess && n >= 1 ? n : otherwise;
}

}  // namespace vtcsweep
