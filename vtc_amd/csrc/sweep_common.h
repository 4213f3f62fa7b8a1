// sweep_common.h -- what the retrieval sweeps share across translation units (sweep_front.hip, sweep_topk.hip, sweep_recall.hip,
// sweep_rank.hip): the ONE function that forms an fp64 distance, and the declarations of the host pieces sweep_front.hip defines.
#pragma once
#include "common.h"

#include <type_traits>

namespace vtcsweep {

// ---- the fp64 squared distance of VTC_SWEEP_EXACT, the recall-only finish and the full-rank sweep --------------------------------------
// One step: four coordinates of a (query, gallery) pair.
__device__ __forceinline__ double dist64_step(const float4 a, const float4 b) {
  const double e0 = (double)a.x - (double)b.x, e1 = (double)a.y - (double)b.y, e2 = (double)a.z - (double)b.z, e3 = (double)a.w - (double)b.w;
  return e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
}
// A lane's piece of a GALLERY row: the four columns at p, as the fp32 values the distance is formed of.  An fp32 row gives them as they
// are (the 16-byte load every caller has always made).  A row stored as IEEE binary16 (the query-time search's half galleries) gives
// the same four columns widened -- 8 bytes loaded, four v_cvt_f32_f16; binary16 -> fp32 is exact, subnormals included, so the float4
// is bit for bit what the fp32 load returns from the widened row and everything after it is shared.
__device__ __forceinline__ float4 row_piece(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 row_piece(const _Float16 *p) {
  typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
  const half4_t h = *reinterpret_cast<const half4_t *>(p);
  return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
// A row stored as 8-bit codes with one fp32 scale (include/vtc_hip.h, "a q8 row"): d signed codes, the scale at byte d, 12 bytes that
// are never read -- d + 16 bytes a row, so FORMING A ROW'S ADDRESS is part of what the element type decides (q8_row).  The value of a
// column is fl32(scale * code), subnormals kept: 4 bytes loaded, four int -> fp32 conversions (exact), four v_mul_f32 -- the float4 is
// bit for bit what the fp32 load returns from the gallery of those products and everything after it is shared.  The scale is not
// part of a piece: the caller loads it once per row, every lane the one address, before the row's first piece (wave_dist64_queries).
struct q8_t {
  signed char code;
};
constexpr int Q8_TAIL = 16;                                // bytes of a row behind its codes: the scale and 12 of padding
struct Q8Piece {
  const q8_t *p;
  float scale;
};
struct Q8Row {
  const q8_t *p;
  float scale;
  __device__ __forceinline__ Q8Piece operator+(int c) const { return {p + c, scale}; }
};
__device__ __forceinline__ const q8_t *q8_row(const q8_t *gallery, long long row, int d) { return gallery + (size_t)row * (size_t)(d + Q8_TAIL); }
__device__ __forceinline__ float q8_scale(const q8_t *row, int d) { return *reinterpret_cast<const float *>(row + d); }
__device__ __forceinline__ float4 row_piece(const Q8Piece g) {
  typedef signed char char4_t __attribute__((ext_vector_type(4)));
  const char4_t c = *reinterpret_cast<const char4_t *>(g.p);
  return make_float4(g.scale * (float)c.x, g.scale * (float)c.y, g.scale * (float)c.z, g.scale * (float)c.w);
}
// fp64 sum_k (q_k - g_k)^2 of NB (query row, gallery row) pairs by the whole wave: qrow(u) / grow(u) are pair u's rows.  Per pair a lane adds
// the steps of its chunks in ascending k, then the xor butterfly leaves every lane with the same bits.  EVERY kernel that forms a distance --
// the re-rank, the fallback, the rescan, the recall-only finish, the full-rank sweep -- does it through this loop (the wrappers below), so a
// distance has the same bits whichever kernel forms it and exact ties stay ties.  All 2 NB row pieces of a K slice are requested before
// the first is used and the NB butterflies interleave: one pair at a time a wave runs a chain of dependent gather latencies.
template <int NB, typename QRow, typename GRow>
__device__ __forceinline__ void wave_dist64_core(QRow qrow, GRow grow, int d, int lane, double (&out)[NB]) {
  double sacc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) sacc[u] = 0.0;
  for (int c = lane * 4; c < d; c += 256) {
    float4 a[NB], b[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      a[u] = *reinterpret_cast<const float4 *>(qrow(u) + c);
      b[u] = row_piece(grow(u) + c);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      sacc[u] += dist64_step(a[u], b[u]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int u = 0; u < NB; ++u) sacc[u] += __shfl_xor(sacc[u], o, 64);
  }
#pragma unroll
  for (int u = 0; u < NB; ++u) out[u] = sacc[u];
}
// one (query, gallery) pair
__device__ __forceinline__ double wave_dist64(const float *__restrict__ q, const float *__restrict__ g, int d, int lane) {
  double out[1];
  wave_dist64_core<1>([&](int) { return q; }, [&](int) { return g; }, d, lane, out);
  return out[0];
}
// one query row against the NB gallery rows jj[] (valid row indices: a caller with absent slots clamps them and drops their results)
template <int NB, typename Idx>
__device__ __forceinline__ void wave_dist64_rows(const float *__restrict__ q, const float *__restrict__ gallery, const Idx (&jj)[NB], int d, int lane,
                                                 double (&out)[NB]) {
  wave_dist64_core<NB>([&](int) { return q; }, [&](int u) { return gallery + (size_t)jj[u] * d; }, d, lane, out);
}
// NB pairs (qs row qi[u], gs row gi[u])
template <int NB>
__device__ __forceinline__ void wave_dist64_pairs(const float *__restrict__ qs, const float *__restrict__ gs, const int (&qi)[NB], const int (&gi)[NB],
                                                  int d, int lane, double (&out)[NB]) {
  wave_dist64_core<NB>([&](int u) { return qs + (size_t)qi[u] * d; }, [&](int u) { return gs + (size_t)gi[u] * d; }, d, lane, out);
}
// the NB consecutive query rows qs[0 .. NB) (row stride d; global memory or LDS) against the NR gallery rows jj[] (valid indices, as above):
// out[u * NR + r] = query u, gallery row jj[r].  The query-time search (search.hip): its tile of queries stays put while the gallery streams by.
// G is the gallery's element type, float or _Float16 (row_piece); the queries are fp32 either way.  G = q8_t: the rows' scales are requested
// first, one load a row that every lane makes of the one address, and ride with the rows into the same loop -- the summation order,
// and so the fp64 bits, of the fp32 gallery of the stored values.
template <int NB, int NR = 1, typename G = float>
__device__ __forceinline__ void wave_dist64_queries(const float *qs, const G *__restrict__ gallery, const int (&jj)[NR], int d, int lane,
                                                    double (&out)[NB * NR]) {
  if constexpr (std::is_same_v<G, q8_t>) {
    Q8Row rows[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      rows[r].p = q8_row(gallery, jj[r], d);
      rows[r].scale = q8_scale(rows[r].p, d);
    }
    wave_dist64_core<NB * NR>([&](int p) { return qs + (size_t)(p / NR) * d; }, [&](int p) { return rows[p % NR]; }, d, lane, out);
  } else {
    wave_dist64_core<NB * NR>([&](int p) { return qs + (size_t)(p / NR) * d; }, [&](int p) { return gallery + (size_t)jj[p % NR] * d; }, d, lane, out);
  }
}

// ---- host pieces, defined in sweep_front.hip ----------------------------------------------------------------------------------------
// |x|^2 of both sets and, for parts = 3 / 1, their split-bf16 operand rows ([hi | lo | hi] queries, [hi | hi | lo] gallery / [hi]); parts = 0: norms only.
// q_rows >= 0: operand rows for the queries [q0, q0 + q_rows) only, qb[0] being row q0's (the norms are still all nq).
void launch_norms_split(const float *queries, int nq, float *qn, bf16_t *qb, const float *gallery, int ng, float *gn, bf16_t *gb, int d, int parts,
                        hipStream_t stream, int q0 = 0, int q_rows = -1);

constexpr int MAX_SEG = 16;   // column segments of a row pass, at most
int default_rows_per_block(int cols);
struct RowSegments {
  int S, seg_cols;
};
RowSegments row_segments(int rows, int cols);

float split_kappa(int d);     // error bound of a BF16X3 distance, relative to |q|^2 + max|g|^2
float exact2_kappa(int d);    // the fp32 terms of a plain-bf16 key's

// the block-minima path
constexpr int RB2 = 128;      // queries per column block: the row block of the phased 256 x 256 tiles' waves
constexpr int CD2 = 64;       // capacity of a candidate list
bool exact2_enabled(int ng, int nq, int depth);
struct Sweep2Ws {
  float *qn, *gn, *gmax, *qmax;      // gmax / qmax: {max |x|^2, max |x~|, max |e|} of the gallery / query side (adjacent 256-byte slots)
  float2 *qst, *gst;                 // (|x~|, |e|) per row
  float *pmax;                       // sweep_prep_kernel's per-block maxima
  bf16_t *qb, *gb;
  unsigned *rowk, *colk;
  int nblk_c, nblk_r;
  int64_t *cand, *cand2;
  int *cand_n, *cand2_n;
  float *theta, *theta2;
  int *flags, *flags2;               // uncertified rows of the row / column direction (count + list)
  size_t total;
};
Sweep2Ws plan2(char *ws, int ng, int nq, int d, bool bidir);
void sweep_prologue(const Sweep2Ws &s, const float *queries, int nq, const float *gallery, int ng, int d, bool round_operands, hipStream_t stream,
                    int *zero_a = nullptr, int *zero_b = nullptr);
void fill_absent_row_blocks(unsigned *colk, int npl, int nblk_pad, int nblk, int n_cols, hipStream_t stream);

// The C ABI's (k_vals, nk): one to four values, each in [1, k_limit]; unused slots are 0.  read_k returns 0, or 1 with the error set (as VTC_CHECK).
struct KList {
  int k[4], nk, kmax;
};
int read_k(KList &kl, const char *fn, const int *k_vals, int nk, int k_limit);

}  // namespace vtcsweep
