// sweep_topk.hip -- the N x N retrieval sweep that returns SORTED LISTS.
//   vtc_l2_topk, vtc_l2_topk_bidir   exact squared-L2 k-NN: replaces faiss.GpuIndexFlatL2.add/search in
//                   RecallAtK.compute (model/metric.py:137-146); both directions from one matrix
//   vtc_l2_sweep_shard_rows / _cols  the same with the rows sharded one process per GPU
//   vtc_recall_hits, vtc_recall_hits_pair   `target in rp[:k]` counting (model/metric.py:148-160)
// Two paths.  The distance-matrix path (every precision; below): WaveList, row / column top-k, merge, and for VTC_SWEEP_EXACT the fp64
// re-rank of the BF16X3 lists with a brute-force fallback.  The block-minima path (VTC_SWEEP_EXACT at >= 1 024 gallery rows, depth <= 32,
// default blocking; "block-minima path" below): no matrix, certified candidate sets from per-block keys, re-rank, rescan.
// The fp64 list, the re-rank and the brute-force scan of both paths' finish are exact_list.h's, shared with the query-time searches.
// The recall-only finish is sweep_recall.hip, the full-rank sweep sweep_rank.hip; what all share, sweep_front.hip / sweep_common.h.
//
// Distance-matrix pipeline (per block of query rows, the fp32 distance matrix "tiled in HBM" as
// BASELINE.json prescribes; blocks of up to 2 GiB):
//   1. row norms |q|^2, |g|^2 in fp32 (once; sweep_front.hip);
//   2. distance GEMM with the L2 epilogue  d = |q|^2 + |g|^2 - 2 q.g  (gemm.hip, EPI_L2DIST):
//        F32     fp32 MFMA, exact;
//        BF16X3  operands split hi/lo into bf16 and concatenated along K
//                ([q_hi|q_lo|q_hi] . [g_hi|g_hi|g_lo]) so that ONE bf16 GEMM with K' = 3D forms
//                q_hi g_hi + q_lo g_hi + q_hi g_lo with fp32 accumulation;
//        BF16    hi parts only;
//   3. streaming top-k: one wave per query row reads the row with 16-byte loads; the wave keeps
//      the sorted best list ONE ENTRY PER LANE; a value is compared against the current k-th best
//      (wave-uniform), so after warm-up almost every step is load + compare + ballot; the rare
//      insertion is a ballot/popcount rank + one shuffle.  Order is (distance, index)
//      lexicographic => ties resolve to the lowest gallery index, independent of scan order.
#include "exact_list.h"

#include <algorithm>

using namespace vtcsweep;

namespace {

// Wave-wide sorted best list, one entry per lane (lane i = i-th best), order = (distance, index).
struct WaveList {
  float bd;
  int bi;
  float tau;     // distance of entry depth-1 (wave-uniform)
  int tau_i;
  __device__ __forceinline__ void init() { bd = INFINITY; bi = 0x7fffffff; tau = INFINITY; tau_i = 0x7fffffff; }
  // offer one candidate per lane (pass = lane has a candidate that beats the current depth-th entry).
  // Insertions are rare after warm-up but serial: broadcasts are v_readlane (the lane index is
  // wave-uniform), the one-lane shift a ds_bpermute.
  __device__ __forceinline__ void offer(float v, int idx, bool pass, int lane, int depth) {
    unsigned long long mask = __ballot(pass);
    while (mask) {
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
      const int ci = __builtin_amdgcn_readlane(idx, l);
      if (cv < tau || (cv == tau && ci < tau_i)) {       // wave-uniform: the list may have tightened meanwhile
        const bool less = (bd < cv) || (bd == cv && bi < ci);
        const int pos = __popcll(__ballot(less));
        // shift by one lane: DPP wave_shr:1 (a VALU move, no LDS round trip as __shfl_up's ds_bpermute)
        const float ud = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, bd), 0x138, 0xf, 0xf, false));
        const int ui = __builtin_amdgcn_update_dpp(0, bi, 0x138, 0xf, 0xf, false);
        if (lane > pos) { bd = ud; bi = ui; }
        if (lane == pos) { bd = cv; bi = ci; }
        tau = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bd), depth - 1));
        tau_i = __builtin_amdgcn_readlane(bi, depth - 1);
      }
    }
  }
  __device__ __forceinline__ bool beats(float v, int idx) const { return v < tau || (v == tau && idx < tau_i); }
};

// One wave per (row, column segment): streams its segment 1024 columns per step -- four 16-byte loads per lane,
// the next TWO steps' loads already in flight while this step is screened (8 KiB per wave outstanding; with the ~2 us
// loaded latency of this path two 16-byte loads per wave and 13 waves per CU left the kernel latency-bound at
// 0.8-1.2 TB/s).  Screening is one min over the lane's 16 values against the wave-uniform k-th best: after
// warm-up almost every step is 4 loads + 15 v_min + 1 ballot.  Segments exist only to put enough waves on the
// chip when a block has few rows; S == 1 writes the final ids/dists directly.
__global__ __launch_bounds__(256) void row_topk_kernel(const float *__restrict__ dist, int ld, int n_rows, int n_cols, int depth,
                                                       int S, int seg_cols, int64_t *__restrict__ ids, float *__restrict__ dists,
                                                       size_t out_row0, float *__restrict__ part_d, int *__restrict__ part_i) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_rows * S) return;
  const int r = w / S, seg = w - r * S;
  const float *row = dist + (size_t)r * ld;
  const int c_lo = seg * seg_cols, c_hi = min(n_cols, c_lo + seg_cols);
  WaveList wl;
  wl.init();
  const bool vec = (ld & 3) == 0;
  // lane's 4 x 4 columns of the step starting at `base`: base + 256 h + 4 lane + e
  auto load_step = [&](int base, float (&v)[16]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = base + 256 * h + lane * 4;
      if (vec && c + 3 < c_hi) {
        typedef float v4f_t __attribute__((ext_vector_type(4)));
        const v4f_t t = __builtin_nontemporal_load(reinterpret_cast<const v4f_t *>(row + c));   // read once
        v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * h + e] = c + e < c_hi ? row[c + e] : INFINITY;
      }
    }
  };
  float cur[16], nxt[16], nx2[16];
  load_step(c_lo, cur);
  if (c_lo + 1024 < c_hi) load_step(c_lo + 1024, nxt);
  for (int base = c_lo; base < c_hi; base += 1024) {
    if (base + 2048 < c_hi) load_step(base + 2048, nx2);     // two steps (8 KiB per wave) in flight behind this one
    float m = cur[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) m = fminf(m, cur[q]);
    // m <= tau is necessary for any of the 16 to beat (tau, tau_i); columns past c_hi hold +inf and never insert
    if (__ballot(m <= wl.tau) != 0ull) {
      if (base == c_lo) {
        // Warm-up: with an empty list every value "beats" it and 1024 candidates would be offered one by one.
        // Offer each lane's smallest first (64 candidates): the list's k-th best is then already within a few
        // ranks of the step's true k-th best and the remaining 960 are screened against it.
        int qm = 0;
#pragma unroll
        for (int q = 1; q < 16; ++q) qm = cur[q] < cur[qm] ? q : qm;     // first minimum = lowest column
        float vm = cur[0];
#pragma unroll
        for (int q = 1; q < 16; ++q) vm = q == qm ? cur[q] : vm;
        const int im = base + 256 * (qm >> 2) + lane * 4 + (qm & 3);
        if (base + 1024 <= c_hi) {
          // a full first step: the 64 lane minima ARE the initial list, sorted by rank counting + one forward
          // permute (as col_topk_kernel) instead of 64 serial insertions
          int rank = 0;
#pragma unroll 4
          for (int l = 0; l < 64; ++l) {
            const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vm), l));
            const int oi = __builtin_amdgcn_readlane(im, l);
            rank += (ov < vm || (ov == vm && oi < im)) ? 1 : 0;
          }
          wl.bd = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(rank << 2, __builtin_bit_cast(int, vm)));
          wl.bi = __builtin_amdgcn_ds_permute(rank << 2, im);
          wl.tau = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl.bd), depth - 1));
          wl.tau_i = __builtin_amdgcn_readlane(wl.bi, depth - 1);
        } else {
          wl.offer(vm, im, im < c_hi, lane, depth);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int idx = base + 256 * (q >> 2) + lane * 4 + (q & 3);
          wl.offer(cur[q], idx, q != qm && idx < c_hi && wl.beats(cur[q], idx), lane, depth);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int idx = base + 256 * (q >> 2) + lane * 4 + (q & 3);
          wl.offer(cur[q], idx, idx < c_hi && wl.beats(cur[q], idx), lane, depth);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) { cur[q] = nxt[q]; nxt[q] = nx2[q]; }
  }
  if (lane < depth) {
    if (S == 1) {
      ids[(out_row0 + r) * depth + lane] = wl.bi == 0x7fffffff ? -1 : (int64_t)wl.bi;
      if (dists) dists[(out_row0 + r) * depth + lane] = wl.bd;
    } else {
      part_d[(size_t)w * depth + lane] = wl.bd;
      part_i[(size_t)w * depth + lane] = wl.bi;
    }
  }
}

// Column direction of the same matrix (the second retrieval direction needs D^T, so it is read off the block
// that the first direction's GEMM has just written instead of running a second GEMM): one workgroup per
// (strip of 64 columns, row segment).  The segment's rows stream through LDS in 64 x 64 tiles (coalesced 256-byte row
// pieces in, 16-byte LDS accesses both ways: row stride 68 floats); wave w owns columns 16w .. 16w+15 of the strip and
// keeps one WaveList per column (2 VGPRs each).  The first tile of a segment initialises a list by rank-counting
// its 64 values (64 serial insertions per column otherwise).  ids are row_id0 + row; partial lists live in
// part[(col * S_total + seg0 + seg) * depth ..], are CARRIED from one block of rows to the next (carry != 0) and are
// merged over segments by topk_merge_kernel.
__global__ __launch_bounds__(256, 4) void col_topk_kernel(const float *__restrict__ dist, int ld, int n_rows, int n_cols, int depth,
                                                       int row_id0, int S, int seg_rows, int S_total, int seg0, int carry,
                                                       float *__restrict__ part_d, int *__restrict__ part_i) {
  __shared__ __attribute__((aligned(16))) float tile[64 * 68];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int strip = blockIdx.x / S, seg = blockIdx.x - strip * S;
  const int c0 = strip * 64;
  const int r_lo = seg * seg_rows, r_hi = min(n_rows, r_lo + seg_rows);
  if (r_lo >= r_hi) {            // empty segment (uniform): its partial lists stay as they are / "invalid"
    if (carry) return;
    for (int cc = 0; cc < 16; ++cc) {
      const int col = c0 + 16 * w + cc;
      if (col < n_cols && lane < depth) {
        part_d[((size_t)col * S_total + seg0 + seg) * depth + lane] = INFINITY;
        part_i[((size_t)col * S_total + seg0 + seg) * depth + lane] = 0x7fffffff;
      }
    }
    return;
  }
  WaveList wl[16];
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    wl[cc].init();
    const int col = c0 + 16 * w + cc;
    if (carry && col < n_cols) {
      // the list of this (column, segment) continues from the previous block of rows: its k-th best is already a
      // tight threshold, so later blocks insert ~k ln(rows_after / rows_before) times instead of ~k ln(rows / 64)
      if (lane < depth) {
        wl[cc].bd = part_d[((size_t)col * S_total + seg0 + seg) * depth + lane];
        wl[cc].bi = part_i[((size_t)col * S_total + seg0 + seg) * depth + lane];
      }
      wl[cc].tau = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl[cc].bd), depth - 1));
      wl[cc].tau_i = __builtin_amdgcn_readlane(wl[cc].bi, depth - 1);
    }
    if (col >= n_cols) wl[cc].tau = -INFINITY;                  // columns past the matrix never offer anything
  }
  const int lr = t >> 4, lc = (t & 15) * 4;
  const bool vec = (ld & 3) == 0 && c0 + 64 <= n_cols;      // uniform: whole strip inside the matrix, rows 16-byte aligned
  auto load_tile = [&](int r_base, float4 (&pre)[4]) {
    if (r_base >= r_hi) return;                              // uniform
    if (vec) {
      // branch-free: rows past the segment re-read its last row and are replaced by +inf, so the four loads of a
      // thread are all in flight together
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int r = r_base + lr + 16 * h;
        pre[h] = *reinterpret_cast<const float4 *>(dist + (size_t)min(r, r_hi - 1) * ld + c0 + lc);
      }
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int r = r_base + lr + 16 * h;
        float4 v = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
        if (r < r_hi) {
          const float *src = dist + (size_t)r * ld + c0 + lc;
          if (c0 + lc < n_cols) v.x = src[0];
          if (c0 + lc + 1 < n_cols) v.y = src[1];
          if (c0 + lc + 2 < n_cols) v.z = src[2];
          if (c0 + lc + 3 < n_cols) v.w = src[3];
        }
        pre[h] = v;
      }
    }
  };
  // one 64-row step: registers -> LDS, refill the registers with the next tile, screen this tile from LDS
  auto step = [&](int r_base, float4 (&pre)[4]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const bool live = r_base + lr + 16 * h < r_hi;
      *reinterpret_cast<float4 *>(tile + (lr + 16 * h) * 68 + lc) =
          make_float4(live ? pre[h].x : INFINITY, live ? pre[h].y : INFINITY, live ? pre[h].z : INFINITY, live ? pre[h].w : INFINITY);
    }
    __syncthreads();
    load_tile(r_base + 64, pre);                             // the next tile is in flight while this one is screened
    const bool valid = r_base + lane < r_hi;
    const int idx = valid ? row_id0 + r_base + lane : 0x7fffffff;
    const bool sort_init = !carry && r_base == r_lo && r_lo + 64 <= r_hi;   // a full first tile of a fresh list (uniform)
    float vv[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t4 = *reinterpret_cast<const float4 *>(tile + lane * 68 + 16 * w + 4 * q);
      vv[4 * q] = t4.x; vv[4 * q + 1] = t4.y; vv[4 * q + 2] = t4.z; vv[4 * q + 3] = t4.w;
    }
    if (sort_init) {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        const float v = vv[cc];
        int rank = 0;
#pragma unroll 4
        for (int l = 0; l < 64; ++l) {
          const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
          const int oi = __builtin_amdgcn_readlane(idx, l);
          rank += (ov < v || (ov == v && oi < idx)) ? 1 : 0;
        }
        // ranks are a permutation (indices are distinct): forward permute = scatter to lane `rank`
        wl[cc].bd = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(rank << 2, __builtin_bit_cast(int, v)));
        wl[cc].bi = __builtin_amdgcn_ds_permute(rank << 2, idx);
        wl[cc].tau = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl[cc].bd), depth - 1));
        wl[cc].tau_i = __builtin_amdgcn_readlane(wl[cc].bi, depth - 1);
        if (c0 + 16 * w + cc >= n_cols) wl[cc].tau = -INFINITY;   // columns past the matrix never offer anything
      }
    } else {
      // hot path: one compare per column, ORed; the per-column control flow runs only when some lane of the wave
      // has a candidate in some column
      bool anyp = false;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) anyp |= vv[cc] <= wl[cc].tau;
      if (__ballot(valid && anyp) != 0ull) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
          wl[cc].offer(vv[cc], idx, valid && vv[cc] <= wl[cc].tau, lane, depth);   // offer() re-checks (tau, tau_i) exactly
      }
    }
    __syncthreads();
  };
  float4 pre[4];
  load_tile(r_lo, pre);
  for (int r_base = r_lo; r_base < r_hi; r_base += 64) step(r_base, pre);
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    const int col = c0 + 16 * w + cc;
    if (col < n_cols && lane < depth) {
      part_d[((size_t)col * S_total + seg0 + seg) * depth + lane] = wl[cc].bd;
      part_i[((size_t)col * S_total + seg0 + seg) * depth + lane] = wl[cc].bi;
    }
  }
}

// One wave per row: merge the S partial lists of the row.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float *__restrict__ part_d, const int *__restrict__ part_i, int n_rows,
                                                         int S, int depth, int64_t *__restrict__ ids, float *__restrict__ dists,
                                                         size_t out_row0) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  WaveList wl;
  wl.init();
  const int total = S * depth;
  for (int base = 0; base < total; base += 64) {
    const int k = base + lane;
    const float v = k < total ? part_d[(size_t)r * total + k] : INFINITY;
    const int idx = k < total ? part_i[(size_t)r * total + k] : 0x7fffffff;
    wl.offer(v, idx, k < total && idx != 0x7fffffff && wl.beats(v, idx), lane, depth);
  }
  if (lane < depth) {
    ids[(out_row0 + r) * depth + lane] = wl.bi == 0x7fffffff ? -1 : (int64_t)wl.bi;
    if (dists) dists[(out_row0 + r) * depth + lane] = wl.bd;
  }
}

// ---- block-minima path: certified candidate sets from the per-block keys of the EPI_L2MIN epilogue ----------------------
// keys[4][nblk][R]: for owner r (a query row; a gallery column in the transposed direction) and block blk of BW gallery
// entries, the three smallest distance keys (the POOL) and the fourth smallest (a bound on everything else in the block).
// With eps_r >= |approx - exact| for every entry of the row:
//   u      = the depth-th smallest pool key of the row     (depth DISTINCT entries lie at or below it, so the exact
//                                                           depth-th distance t satisfies t <= u + eps)
//   theta  = u + 2 eps                                      (every true top-depth entry has approx <= t + eps <= theta)
//   C_r    = all pool entries with key <= theta             (the candidate set handed to the fp64 re-rank)
//   proof of completeness: if the smallest fourth-in-block key of the row is > theta, no entry outside the pool can have
//   approx <= theta, hence C_r contains every entry with approx <= theta, hence the true top-depth.  Otherwise (or if
//   |C_r| > 64) cand_n[r] = -1 and the row is recomputed by fp64 brute force.
// One workgroup per 64 owners; blocks of 64 x 64 keys are transposed through LDS (coalesced 256-byte reads in, one
// owner's 64 keys per wave read out).  Pass 1 reads plane 0 only (u is taken over block minima: still depth distinct
// entries, a valid if slightly larger u); pass 2 reads all four planes and emits C_r with ballot compaction.
// Key layout: keys[src][plane][block-of-src][owner] with `nbs` blocks per source (one source: the planes of a local GEMM,
// nbs == nblk; several: the column planes every rank sent for this rank's columns, stacked in rank order) -- block `blk`
// holds entries src_base[blk / nbs] + (blk % nbs) * bw + (key & 127) of the other side (src_base == NULL: 0).
// OW owners per workgroup: 64, or 32 when 64 would leave CUs without a workgroup (10k x 10k: 157 workgroups of 64)
// (round 4: ONE launch serves both directions of the one-matrix sweep -- workgroups [0, nblocks_a) take problem A, the rest B;
// nblocks_a == gridDim.x: a single problem.  The same holds for exact_rerank_kernel and block_rescan_kernel below.)
struct MinselArgs {
  const unsigned *keys;
  int R, nblk, bw, nbs;
  const int *src_base;
  int depth;
  const float *own_norm;
  const float2 *own_st;
  const float *other_max;
  float kappa;
  int64_t *cand;
  int *cand_n;
  float *theta_out;
};
template <int OW>
__global__ __launch_bounds__(256) void minsel_kernel(const MinselArgs PA, const MinselArgs PB, int nblocks_a) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const MinselArgs &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const unsigned *__restrict__ keys = P.keys;
  const int R = P.R, nblk = P.nblk, bw = P.bw, nbs = P.nbs, depth = P.depth;
  const int *__restrict__ src_base = P.src_base;
  const float *__restrict__ own_norm = P.own_norm;
  const float2 *__restrict__ own_st = P.own_st;
  const float *__restrict__ other_max = P.other_max;
  const float kappa = P.kappa;
  int64_t *__restrict__ cand = P.cand;
  int *__restrict__ cand_n = P.cand_n;
  float *__restrict__ theta_out = P.theta_out;
  constexpr int TG = OW / 4, NSUB = 256 / TG, NI = 64 / NSUB;      // vector loads: TG threads along the owners, NSUB block slices
  constexpr int OPW = OW / 4;                                       // owners per wave
  constexpr int SROWS = 256 / OW, NQ = 64 / SROWS;                  // scalar loads: a thread per owner, SROWS block slices
  static_assert(OW == 64 || OW == 32, "owners per workgroup");
  __shared__ unsigned tl[3][64 * 65];
  __shared__ float bmin[32][64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int r0 = bid * OW;
  const size_t plane = (size_t)nbs * R;                       // one plane of one source
  auto blk_off = [&](int blk) -> size_t {                      // offset of (plane 0, blk, owner 0)
    const int src = blk / nbs;
    return ((size_t)src * (L2MIN_PLANES - 1) * nbs + blk) * R;   // = ((src * 4) * nbs + blk % nbs) * R
  };
  const int so = t % OW, sb = t / OW;                           // scalar loads: this thread's owner and block slice
  const bool rv = r0 + so < R;
  const float INF = __builtin_bit_cast(float, 0x7F800000u);
  // ---- pass 1: per owner, the two smallest block minima each lane has seen ----
  float m1[OPW], m2[OPW];
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) m1[cc] = m2[cc] = INF;
  // tile loads: 16-byte loads (four consecutive owners per thread, all of a chunk's loads in flight at once) when the
  // planes' rows are 16-byte aligned, else one key per thread
  const bool vec = (R & 3) == 0;
  const int og = 4 * (t % TG), sub = t / TG;
  float bq[4] = {INF, INF, INF, INF};
  auto load_chunk = [&](int c0, int npl) __attribute__((always_inline)) {
    if (vec) {
      uint4 v[NI][4];
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        const int blk = c0 + sub + NSUB * it;
        const bool ok = blk < nblk && r0 + og < R;
        const size_t o = (ok ? blk_off(blk) : 0) + r0 + og;
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
          if (pl < npl) v[it][pl] = ok ? *reinterpret_cast<const uint4 *>(keys + pl * plane + o) : make_uint4(0x7F800000u, 0x7F800000u, 0x7F800000u, 0x7F800000u);
      }
#pragma unroll
      for (int it = 0; it < NI; ++it) {
        const int bl = sub + NSUB * it;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          if (pl < npl) {
            tl[pl][bl * 65 + og + 0] = v[it][pl].x; tl[pl][bl * 65 + og + 1] = v[it][pl].y;
            tl[pl][bl * 65 + og + 2] = v[it][pl].z; tl[pl][bl * 65 + og + 3] = v[it][pl].w;
          }
        if (npl == 4) {     // fourth-in-block keys: running min per owner, reduced over the threads at the end
          bq[0] = fminf(bq[0], __uint_as_float(v[it][3].x)); bq[1] = fminf(bq[1], __uint_as_float(v[it][3].y));
          bq[2] = fminf(bq[2], __uint_as_float(v[it][3].z)); bq[3] = fminf(bq[3], __uint_as_float(v[it][3].w));
        }
      }
    } else {
#pragma unroll 4
      for (int q = 0; q < NQ; ++q) {
        const int bl = sb + SROWS * q, blk = c0 + bl;
        const bool ok = blk < nblk && rv;
        const size_t o = (ok ? blk_off(blk) : 0) + r0 + so;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          if (pl < npl) tl[pl][bl * 65 + so] = ok ? keys[pl * plane + o] : 0x7F800000u;
        if (npl == 4 && ok) bq[0] = fminf(bq[0], __uint_as_float(keys[3 * plane + o]));
      }
    }
  };
  for (int c0 = 0; c0 < nblk; c0 += 64) {
    load_chunk(c0, 1);
    __syncthreads();
#pragma unroll
    for (int cc = 0; cc < OPW; ++cc) {
      const float k = __uint_as_float(tl[0][lane * 65 + OPW * w + cc]);
      m2[cc] = fminf(m2[cc], fmaxf(m1[cc], k));
      m1[cc] = fminf(m1[cc], k);
    }
    __syncthreads();
  }
  // depth-th smallest of the wave's 128 values per owner: the 64 lane minima sorted by rank counting, then the few second
  // minima that beat the running depth-th
  float theta[OPW];
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) {
    const float v = m1[cc];
    int rank = 0;
#pragma unroll 4
    for (int l = 0; l < 64; ++l) {
      const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
      rank += (ov < v || (ov == v && l < lane)) ? 1 : 0;
    }
    WaveList wl;
    wl.bd = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(rank << 2, __builtin_bit_cast(int, v)));
    wl.bi = __builtin_amdgcn_ds_permute(rank << 2, lane);
    wl.tau = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wl.bd), depth - 1));
    wl.tau_i = __builtin_amdgcn_readlane(wl.bi, depth - 1);
    wl.offer(m2[cc], 64 + lane, wl.beats(m2[cc], 64 + lane), lane, depth);
    const float u = wl.tau;
    const int r = min(r0 + OPW * w + cc, R - 1);
    // |approx - exact| of any entry of this owner's row (sweep_prep_kernel: measured rounding errors; other_max = the other
    // side's {max |x|^2, max |x~|, max |e|}) + kappa x the fp32 terms (accumulation, norms, the key's index bits)
    const float2 st = own_st[r];
    const float eps = 1.001f * (2.0f * (st.x * other_max[2] + st.y * other_max[1] + st.y * other_max[2]) + kappa * (own_norm[r] + other_max[0]));
    theta[cc] = u + 2.0f * eps;          // u == +inf (fewer than depth pool entries) keeps theta infinite: everything is a candidate
  }
  // ---- pass 2: every pool entry with key <= theta, and the smallest fourth-in-block key ----
  int cnt[OPW];
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) cnt[cc] = 0;
  for (int c0 = 0; c0 < nblk; c0 += 64) {
    load_chunk(c0, 4);
    __syncthreads();
    const int blk = c0 + lane;
    const int64_t base = blk < nblk ? (int64_t)(src_base ? src_base[blk / nbs] : 0) + (int64_t)(blk % nbs) * bw : 0;
#pragma unroll
    for (int cc = 0; cc < OPW; ++cc) {
      const int o = OPW * w + cc;
      const int r = r0 + o;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const unsigned k = tl[pl][lane * 65 + o];
        const bool pass = __uint_as_float(k & ~127u) <= theta[cc] && k != 0x7F800000u;
        const unsigned long long mask = __ballot(pass);
        if (mask) {                                                       // wave-uniform
          const int pos = cnt[cc] + __popcll(mask & ((1ull << lane) - 1ull));
          if (pass && pos < 64 && r < R) cand[(size_t)r * 64 + pos] = base + (int)(k & 127u);
          cnt[cc] += __popcll(mask);
        }
      }
    }
    __syncthreads();
  }
  // smallest fourth-in-block key per owner: the threads' running minima -> bmin[slice][owner] -> min over the slices
  for (int i = t; i < 32 * 64; i += 256) (&bmin[0][0])[i] = INF;
  __syncthreads();
  if (vec) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bmin[sub][og + e] = bq[e];
  } else {
    bmin[sb][so] = bq[0];
  }
  __syncthreads();
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) {
    const int o = OPW * w + cc, r = r0 + o;
    if (r < R && lane == 0) {
      float bound = INF;
      for (int sl = 0; sl < 32; ++sl) bound = fminf(bound, bmin[sl][o]);
      // strict: an outside entry AT theta could tie with a true neighbour
      cand_n[r] = (cnt[cc] <= 64 && bound > theta[cc]) ? cnt[cc] : -1;
      theta_out[r] = theta[cc];                            // for the uncertified owners' second pass (block_rescan_kernel)
    }
  }
}

static MinselArgs minsel_args(const unsigned *keys, int R, int nblk, int bw, int nbs, const int *src_base, int depth, const float *own_norm,
                              const float2 *own_st, const float *other_max, float kappa, int64_t *cand, int *cand_n, float *theta) {
  return MinselArgs{keys, R, nblk, bw, nbs, src_base, depth, own_norm, own_st, other_max, kappa, cand, cand_n, theta};
}
// one problem (B == nullptr) or both directions in one launch
static void launch_minsel(const MinselArgs &A, const MinselArgs *B, hipStream_t stream) {
  const int total = A.R + (B ? B->R : 0);
  const MinselArgs &Bv = B ? *B : A;
  if (cdiv(total, 64) < vtcgemm::num_cus()) {
    const int na = cdiv(A.R, 32), nb = B ? cdiv(B->R, 32) : 0;
    hipLaunchKernelGGL(minsel_kernel<32>, dim3(na + nb), dim3(256), 0, stream, A, Bv, na);
  } else {
    const int na = cdiv(A.R, 64), nb = B ? cdiv(B->R, 64) : 0;
    hipLaunchKernelGGL(minsel_kernel<64>, dim3(na + nb), dim3(256), 0, stream, A, Bv, na);
  }
}

// ---- VTC_SWEEP_EXACT: fp64 finish of both paths' candidate lists (distances: sweep_common.h) ------------------------------------------
// One wave per query row: fp64 distances of the row's `cdepth` BF16X3 candidates, sorted by (distance, index); the
// first `depth` are the answer IF the candidate list provably contains the true top-`depth`: every true member j
// has approx(j) <= approx_(depth) + 2 eps, so it is on the list when approx_(cdepth) > approx_(depth) + 2 eps, with
// eps = split_kappa (|q|^2 + max|g|^2) a worst-case bound of the split-bf16 distance error (dropped lo.lo products, the
// two bf16 roundings of each operand, fp32 accumulation of 3 D products).  Otherwise the row is flagged.
struct RerankArgs {
  const float *queries, *gallery;
  int nq, ng, d;
  const int64_t *cand;
  const float *cand_d;
  int cdepth, depth;
  const float *qn, *gmax;
  float kappa;
  int64_t *ids;
  float *dists;
  int *flags;          // flags[0] = count, flags[1..] = rows
  const int *cand_n;   // block-minima path: the row's list holds cand_n[r] entries and is ALREADY certified complete (< 0: it is not); else nullptr
};
__global__ __launch_bounds__(256) void exact_rerank_kernel(const RerankArgs PA, const RerankArgs PB, int nblocks_a) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const RerankArgs &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const float *__restrict__ queries = P.queries, *__restrict__ gallery = P.gallery;
  const int nq = P.nq, ng = P.ng, d = P.d, cdepth = P.cdepth, depth = P.depth;
  const int64_t *__restrict__ cand = P.cand;
  const float *__restrict__ cand_d = P.cand_d, *__restrict__ qn = P.qn, *__restrict__ gmax = P.gmax;
  const float kappa = P.kappa;
  int64_t *__restrict__ ids = P.ids;
  float *__restrict__ dists = P.dists;
  int *__restrict__ flags = P.flags;
  const int *__restrict__ cand_n = P.cand_n;
  const int lane = threadIdx.x & 63;
  const int r = bid * 4 + (threadIdx.x >> 6);
  if (r >= nq) return;
  const float *q = queries + (size_t)r * d;
  const int n_list = cand_n ? cand_n[r] : cdepth;
  const int64_t my = lane < n_list ? cand[(size_t)r * cdepth + lane] : -1;
  const int n_loop = cand_n ? (n_list > 0 ? n_list : 0) : cdepth;      // wave-uniform
  double md;
  const int rank = rerank64(q, gallery, (long long)my, n_loop, d, lane, md);
  if (lane < cdepth && my >= 0 && rank < depth) {
    ids[(size_t)r * depth + rank] = my;
    if (dists) dists[(size_t)r * depth + rank] = (float)md;
  }
  const int n_valid = __popcll(__ballot(my >= 0));
  if (lane == 0) {
    bool sure = n_valid >= ng;                            // the list IS the gallery
    if (cand_n) {
      sure = sure || n_valid >= depth;                    // certified by minsel_kernel (n_list < 0 -> n_valid == 0)
    } else if (!sure && n_valid >= depth) {
      const float eps = kappa * (qn[r] + *gmax);
      // everything outside the list is at least as far (approx) as its last entry
      const float outside = n_valid >= cdepth ? cand_d[(size_t)r * cdepth + cdepth - 1] : INFINITY;
      sure = outside > cand_d[(size_t)r * cdepth + depth - 1] + 2.0f * eps;
    }
    if (!sure) flags[1 + atomicAdd(flags, 1)] = r;
  }
}

// Flagged rows only (dense near-ties: duplicates in the gallery): fp64 brute force over the whole gallery, one workgroup per row
// (fallback_scan, exact_list.h; a gallery row at +inf is a row).
__global__ __launch_bounds__(256) void exact_fallback_kernel(const float *__restrict__ queries, const float *__restrict__ gallery, int ng,
                                                             int d, int depth, const int *__restrict__ flags, int64_t *__restrict__ ids,
                                                             float *__restrict__ dists) {
  __shared__ double sd[4][64];
  __shared__ long long si[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_flagged = flags[0];
  for (int f = blockIdx.x; f < n_flagged; f += gridDim.x) {   // uniform for the workgroup; normally zero trips
    const int r = flags[1 + f];
    const auto m = fallback_scan<false, 4>(queries + (size_t)r * d, gallery, nullptr, ng, d, depth, &sd[0][0], &si[0][0]);
    if (wave == 0) write_result_row(m, r, depth, lane, 0, ids, dists, nullptr);
    __syncthreads();                                         // sd / si are reused by the next flagged row
  }
}

// Uncertified owners of the block-minima path (minsel_kernel: more than 64 pool entries under theta, or a block whose fourth
// smallest key is under theta and may hide more): instead of the whole gallery, exactly the entries that CAN be under theta --
// the pool entries <= theta of the safe blocks and EVERY entry of the unsafe ones (an entry that is not among its block's three
// smallest has the block's fourth key below its own).  That set contains the true top-depth; fp64 distances, sorted by
// (distance, index): the same ids as the brute force.  One workgroup per flagged owner, a wave per block at a time.
struct RescanArgs {
  const float *queries, *gallery;
  int ng, d, depth;
  const int *flags;
  const unsigned *keys;
  int R, nblk, bw, nbs, n_src;
  const int *src_base;
  const float *theta;
  int64_t *ids;
  float *dists;
};
__global__ __launch_bounds__(256) void block_rescan_kernel(const RescanArgs PA, const RescanArgs PB, int nblocks_a) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const RescanArgs &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const int nbl = second ? (int)gridDim.x - nblocks_a : nblocks_a;
  const float *__restrict__ queries = P.queries, *__restrict__ gallery = P.gallery;
  const int ng = P.ng, d = P.d, depth = P.depth, R = P.R, nblk = P.nblk, bw = P.bw, nbs = P.nbs, n_src = P.n_src;
  const int *__restrict__ flags = P.flags;
  const unsigned *__restrict__ keys = P.keys;
  const int *__restrict__ src_base = P.src_base;
  const float *__restrict__ theta = P.theta;
  int64_t *__restrict__ ids = P.ids;
  float *__restrict__ dists = P.dists;
  constexpr int CAP = 4096;               // candidate list of a round: CAP / bw blocks, each at most bw entries
  __shared__ double sd[4][64];
  __shared__ int si[4][64];
  __shared__ int clist[CAP];
  __shared__ int cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_flagged = flags[0];
  const size_t plane = (size_t)nbs * R;
  const int cb = min(CAP / bw, 256);      // blocks per round, a thread per block
  for (int f = bid; f < n_flagged; f += nbl) {     // uniform for the workgroup
    const int r = flags[1 + f];
    const float *q = queries + (size_t)r * d;
    const float th = theta[r];
    SortedList<int, EMPTY_ROW, false> wl;
    wl.init();
    for (int blk0 = 0; blk0 < nblk; blk0 += cb) {
      if (tid == 0) cnt = 0;
      __syncthreads();
      // list the round's candidates: a thread per block, its four keys fetched at once
      const int blk = blk0 + tid;
      if (tid < cb && blk < nblk) {
        const int src = blk / nbs, b_in = blk - src * nbs;
        const size_t o = ((size_t)src * (L2MIN_PLANES - 1) * nbs + blk) * R + r;
        unsigned kk[4];
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) kk[pl] = keys[pl * plane + o];
        const int base = (src_base ? src_base[src] : 0) + b_in * bw;
        const int lim = (src_base && src + 1 < n_src) ? src_base[src + 1] : ng;     // the source's rows end here
        if (kk[3] != 0x7F800000u && __uint_as_float(kk[3] & ~127u) <= th) {           // unsafe block: every entry
          const int n_in = min(bw, lim - base);
          if (n_in > 0) {
            const int pos = atomicAdd(&cnt, n_in);
            for (int j = 0; j < n_in; ++j) clist[pos + j] = base + j;
          }
        } else {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            if (kk[pl] != 0x7F800000u && __uint_as_float(kk[pl] & ~127u) <= th) clist[atomicAdd(&cnt, 1)] = base + (int)(kk[pl] & 127u);
        }
      }
      __syncthreads();
      // fp64 distances, four gallery rows per step and wave (their loads in flight together); the order of the offers does not matter
      const int n_list = cnt;
      for (int c0 = 4 * wave; c0 < n_list; c0 += 16) {
        int jj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) jj[u] = clist[min(c0 + u, n_list - 1)];
        double sacc[4];
        wave_dist64_rows(q, gallery, jj, d, lane, sacc);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c0 + u < n_list) wl.offer<false>(sacc[u], jj[u], 0, lane, depth);
      }
      __syncthreads();
    }
    sd[wave][lane] = wl.bd;
    si[wave][lane] = wl.bi;
    __syncthreads();
    if (wave == 0) {
      SortedList<int, EMPTY_ROW, false> m;
      m.init();
      merge_lists<false>(m, LdsLists<int>{&sd[0][0], &si[0][0], nullptr}, 4, 0, 64, depth, lane);
      write_result_row(m, r, depth, lane, 0, ids, dists, nullptr);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void max_reduce_kernel(const float *__restrict__ x, int n, float *__restrict__ out) {
  __shared__ float part[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, x[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// (ids2 != NULL: a second id array of the same shape and targets -- the other direction -- counted into hits2 by the second half of the grid)
__global__ __launch_bounds__(256) void recall_hits_kernel(const int64_t *__restrict__ ids, int n, int depth, int64_t target_offset,
                                                          int k0, int k1, int k2, int k3, int nk, unsigned long long *hits,
                                                          const int64_t *__restrict__ ids2, unsigned long long *hits2) {
  const int half = (int)gridDim.x >> (ids2 ? 1 : 0);
  if (ids2 && (int)blockIdx.x >= half) { ids = ids2; hits = hits2; }
  const int i = ((int)blockIdx.x % half) * 256 + threadIdx.x;
  int rank = 1 << 30;
  if (i < n) {
    const int64_t t = target_offset + i;
    for (int j = 0; j < depth; ++j)
      if (ids[(size_t)i * depth + j] == t) { rank = j; break; }
  }
  const int ks[4] = {k0, k1, k2, k3};
  for (int q = 0; q < nk; ++q) {
    const bool hit = i < n && rank < ks[q];
    const int cnt = __popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&hits[q], (unsigned long long)cnt);
  }
}

struct SweepWs {
  float *qn, *gn;
  bf16_t *qb, *gb;
  float *dist;
  float *part_d;
  int *part_i;
  int rows_per_block;
  // VTC_SWEEP_EXACT only
  int64_t *cand;
  float *cand_d, *gmax;
  int *flags;
  int cdepth;
  // both directions from one matrix (vtc_l2_topk_bidir): partial column lists, and the EXACT mode's second candidate set
  float *cpart_d;
  int *cpart_i;
  int c_seg, c_total;            // row segments per block = partial lists per column (carried across blocks)
  int64_t *cand2;
  float *cand2_d, *qmax;
  size_t total;
};
constexpr int MAX_CSEG = 8;

SweepWs plan(char *ws, int ng, int nq, int d, int precision, int rows_per_block, bool bidir = false) {
  SweepWs s;
  const bool exact = precision == VTC_SWEEP_EXACT;
  if (exact) precision = VTC_SWEEP_BF16X3;
  Bump b(ws);
  auto take = [&](size_t bytes) { return b.take(bytes); };
  s.qn = (float *)take((size_t)nq * 4);
  s.gn = (float *)take((size_t)ng * 4);
  const int parts = precision == VTC_SWEEP_BF16X3 ? 3 : (precision == VTC_SWEEP_BF16 ? 1 : 0);
  s.qb = (bf16_t *)take((size_t)nq * d * parts * 2);
  s.gb = (bf16_t *)take((size_t)ng * d * parts * 2);
  int rpb = rows_per_block;
  if (rpb <= 0) rpb = default_rows_per_block(ng);
  if (rpb > nq) rpb = nq;
  s.rows_per_block = rpb;
  s.dist = (float *)take((size_t)rpb * ng * 4);
  s.part_d = (float *)take((size_t)rpb * MAX_SEG * 64 * 4);
  s.part_i = (int *)take((size_t)rpb * MAX_SEG * 64 * 4);
  s.cand = nullptr; s.cand_d = nullptr; s.gmax = nullptr; s.flags = nullptr; s.cdepth = 0;
  if (exact) {
    s.cdepth = 64;                                          // sized for the deepest list (depth is not known to the size query)
    s.cand = (int64_t *)take((size_t)nq * 64 * 8);
    s.cand_d = (float *)take((size_t)nq * 64 * 4);
    s.flags = (int *)take((size_t)(std::max(nq, bidir ? ng : 0) + 1) * 4);   // [0] = number of flagged rows, then their indices
    s.gmax = (float *)take(256);
  }
  s.cpart_d = nullptr; s.cpart_i = nullptr; s.cand2 = nullptr; s.cand2_d = nullptr; s.qmax = nullptr; s.c_seg = 0; s.c_total = 0;
  if (bidir) {
    // enough (strip, segment) workgroups to fill the chip: ~4 per CU
    const int strips = cdiv(ng, 64);
    // (strip, segment) workgroups, four resident per CU: the fewest segments that put ~3 workgroups on every CU --
    // the pass is bound by instruction issue, and every extra segment costs a list initialisation plus its own early
    // insertions (measured at 50k x 50k: 1 / 2 / 3 / 5 segments per block = 4.3 / 4.6 / 5.1 / 6.2 ms per direction)
    s.c_seg = std::max(1, std::min(MAX_CSEG, cdiv(3 * vtcgemm::num_cus(), strips)));
    s.c_seg = std::min(s.c_seg, std::max(1, rpb / 128));                    // at least two tiles per segment
    s.c_total = s.c_seg;                                     // a (column, segment) list is carried from block to block
    s.cpart_d = (float *)take((size_t)ng * s.c_total * 64 * 4);
    s.cpart_i = (int *)take((size_t)ng * s.c_total * 64 * 4);
    if (exact) {
      s.cand2 = (int64_t *)take((size_t)ng * 64 * 8);
      s.cand2_d = (float *)take((size_t)ng * 64 * 4);
      s.qmax = (float *)take(256);
    }
  }
  s.total = b.off;
  return s;
}

// col_ids != nullptr: also the transposed direction (for every gallery row its nearest query rows), read off the same
// distance blocks by col_topk_kernel.
static int l2_topk_impl(const float *gallery, const float *queries, int ng, int nq, int d, int depth, int precision,
                        int64_t *ids, float *dists, const SweepWs &s, hipStream_t stream, int64_t *col_ids = nullptr,
                        float *col_dists = nullptr) {
  const int parts = precision == VTC_SWEEP_BF16X3 ? 3 : 1;
  launch_norms_split(queries, nq, s.qn, s.qb, gallery, ng, s.gn, s.gb, d, precision == VTC_SWEEP_F32 ? 0 : parts, stream);
  VTC_LAUNCH_CHECK("l2_topk prologue");
  for (int r0 = 0; r0 < nq; r0 += s.rows_per_block) {
    const int rows = min(s.rows_per_block, nq - r0);
    GemmEpi e;
    e.mode = EPI_L2DIST; e.out_dtype = VTC_F32; e.rown = s.qn + r0; e.coln = s.gn;
    int rc;
    if (precision == VTC_SWEEP_F32)
      rc = launch_gemm(queries + (size_t)r0 * d, gallery, nullptr, s.dist, rows, ng, d, VTC_F32, e, stream);
    else
      rc = launch_gemm(s.qb + (size_t)r0 * d * parts, s.gb, nullptr, s.dist, rows, ng, d * parts, VTC_BF16, e, stream);
    if (rc) return rc;
    {
      const auto [S, seg_cols] = row_segments(rows, ng);
      ProfScope prof(VTC_PROF_TOPK, (double)rows * ng * 4, stream);
      hipLaunchKernelGGL(row_topk_kernel, dim3(cdiv(rows * S, 4)), dim3(256), 0, stream, s.dist, ng, rows, ng, depth, S, seg_cols, ids,
                         dists, (size_t)r0, s.part_d, s.part_i);
      if (S > 1)
        hipLaunchKernelGGL(topk_merge_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, stream, s.part_d, s.part_i, rows, S, depth, ids, dists,
                           (size_t)r0);
    }
    VTC_LAUNCH_CHECK("row_topk");
    if (col_ids) {
      const int seg_rows = cdiv(cdiv(rows, s.c_seg), 64) * 64;
      ProfScope prof(VTC_PROF_TOPK, (double)rows * ng * 4, stream);
      hipLaunchKernelGGL(col_topk_kernel, dim3(cdiv(ng, 64) * s.c_seg), dim3(256), 0, stream, s.dist, ng, rows, ng, depth, r0, s.c_seg,
                         seg_rows, s.c_total, 0, r0 > 0 ? 1 : 0, s.cpart_d, s.cpart_i);
      VTC_LAUNCH_CHECK("col_topk");
    }
  }
  if (col_ids) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3(cdiv(ng, 4)), dim3(256), 0, stream, s.cpart_d, s.cpart_i, ng, s.c_total, depth, col_ids,
                       col_dists, (size_t)0);
    VTC_LAUNCH_CHECK("col_topk merge");
  }
  return 0;
}

// EXACT tail of the split-bf16 candidate lists (galleries under 1 024 rows, depth over 32): re-rank the lists with fp64 distances,
// accept the rows whose list provably holds the true top-k, recompute the others by fp64 brute force.  qn / gn: fp32 squared norms
// of the queries / gallery rows.
static int exact_finish_lists(const float *gallery, const float *queries, int ng, int nq, int d, int depth, int cdepth, const int64_t *cand,
                              const float *cand_d, const float *qn, const float *gn, float *gmax, int *flags, int64_t *ids, float *dists,
                              hipStream_t stream) {
  hipLaunchKernelGGL(max_reduce_kernel, dim3(1), dim3(256), 0, stream, gn, ng, gmax);
  const float kappa = split_kappa(d);
  (void)hipMemsetAsync(flags, 0, sizeof(int), stream);
  const RerankArgs ra{queries, gallery, nq, ng, d, cand, cand_d, cdepth, depth, qn, gmax, kappa, ids, dists, flags, nullptr};
  {   // (work = bytes gathered at ~2 x depth candidates per row: the lists' lengths live on the device)
    ProfScope prof(VTC_PROF_TOPK, (double)nq * (2.0 * depth + 1.0) * d * 4, stream);
    hipLaunchKernelGGL(exact_rerank_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, stream, ra, ra, cdiv(nq, 4));
  }
  hipLaunchKernelGGL(exact_fallback_kernel, dim3(std::min(nq, 2048)), dim3(256), 0, stream, queries, gallery, ng, d, depth, flags, ids, dists);
  VTC_LAUNCH_CHECK("l2_topk exact");
  return 0;
}

// ---- VTC_SWEEP_EXACT, block-minima path ("v2") -----------------------------------------------------------------------
// ONE plain-bf16 distance GEMM whose epilogue keeps, per (query, block of 64 gallery rows), the three smallest distances and
// the fourth as a bound (gemm.hip, EPI_L2MIN) -- and, for vtc_l2_topk_bidir, the same per (gallery row, block of RB queries)
// from the same accumulators; no N x N matrix is written or read.  minsel_kernel turns the block minima into a candidate set
// that provably (given the per-entry error bound exact2_kappa, derived there) contains the query's true top-k (or says that it cannot), exact_rerank_kernel orders it by fp64 distances,
// the uncertified queries are settled from their own planes (block_rescan_kernel).

// Finish of the CERTIFIED candidate lists (minsel_kernel): fp64 re-rank, then the uncertified owners are settled from their own planes
// (block_rescan_kernel: no pass over the gallery).  One problem (B == nullptr) or both directions in one launch per stage (rounds 2-3:
// two) -- the stages of the two directions are independent, and at 10k x 10k a direction alone leaves CUs idle (a re-rank wave per row).
struct Certified {
  RescanArgs rs;           // the direction's problem, key planes and outputs
  const int64_t *cand;     // [R][CD2] candidate lists
  const int *cand_n;       // their lengths (< 0: not certified)
  int *flags;              // = rs.flags, writable: the re-rank lists the uncertified owners there
};
int certified_finish(const Certified &A, const Certified *B, hipStream_t stream) {
  auto rerank_args = [](const Certified &c) {     // (certified lists carry no error bound: cand_d, qn, gmax and kappa are not read)
    return RerankArgs{c.rs.queries, c.rs.gallery, c.rs.R, c.rs.ng, c.rs.d, c.cand, nullptr, CD2, c.rs.depth, nullptr, nullptr, 0.f,
                      c.rs.ids, c.rs.dists, c.flags, c.cand_n};
  };
  const Certified &Bv = B ? *B : A;
  // both counters: one fill (B's flags lie behind A's in the plan; the lists between them are rewritten anyway)
  (void)hipMemsetAsync(A.flags, 0, (size_t)((char *)Bv.flags - (char *)A.flags) + sizeof(int), stream);
  {   // (work = bytes gathered at ~2 x depth candidates per row: the lists' lengths live on the device)
    ProfScope prof(VTC_PROF_TOPK, (double)(A.rs.R + (B ? B->rs.R : 0)) * (2.0 * A.rs.depth + 1.0) * A.rs.d * 4, stream);
    const int na = cdiv(A.rs.R, 4), nb = B ? cdiv(B->rs.R, 4) : 0;
    hipLaunchKernelGGL(exact_rerank_kernel, dim3(na + nb), dim3(256), 0, stream, rerank_args(A), rerank_args(Bv), na);
  }
  {
    ProfScope prof(VTC_PROF_TOPK, 0.0, stream);
    const int cap = B ? 1024 : 2048;
    const int ga = std::min(A.rs.R, cap), gb = B ? std::min(B->rs.R, cap) : 0;
    hipLaunchKernelGGL(block_rescan_kernel, dim3(ga + gb), dim3(256), 0, stream, A.rs, Bv.rs, ga);
  }
  VTC_LAUNCH_CHECK("l2_topk exact (certified lists)");
  return 0;
}

// gallery a [na], queries b [nb]; ids_a2b != nullptr: also the transposed direction
// colk_out != NULL (sharded sweep, rank-local rows): the column planes go to the caller's [4, nblk_r_pad, na] buffer and the
// column direction is NOT finished here (vtc_l2_sweep_shard_cols does, after the exchange)
int exact2_impl(const float *a, const float *b, int na, int nb, int d, int depth, int64_t *ids_b2a, float *dists_b2a, int64_t *ids_a2b,
                float *dists_a2b, const Sweep2Ws &s, hipStream_t stream, unsigned *colk_out = nullptr, int nblk_r_pad = 0) {
  sweep_prologue(s, b, nb, a, na, d, true, stream);
  VTC_LAUNCH_CHECK("l2_topk prologue");
  GemmEpi e;
  e.mode = EPI_L2MIN; e.out_dtype = VTC_F32; e.rown = s.qn; e.coln = s.gn;
  e.rowk = s.rowk; e.colk = ids_a2b ? s.colk : nullptr; e.nblk_c = s.nblk_c; e.nblk_r = s.nblk_r;
  if (colk_out) {
    e.colk = colk_out; e.nblk_r = nblk_r_pad;
    fill_absent_row_blocks(colk_out, L2MIN_PLANES, nblk_r_pad, s.nblk_r, na, stream);
  }
  if (int rc = launch_gemm(s.qb, s.gb, nullptr, nullptr, nb, na, d, VTC_BF16, e, stream)) return rc;
  const float kappa = exact2_kappa(d);
  const MinselArgs m1 = minsel_args(s.rowk, nb, s.nblk_c, 64, s.nblk_c, nullptr, depth, s.qn, s.qst, s.gmax, kappa, s.cand, s.cand_n, s.theta);
  const Certified c1{{b, a, na, d, depth, s.flags, s.rowk, nb, s.nblk_c, 64, s.nblk_c, 1, nullptr, s.theta, ids_b2a, dists_b2a}, s.cand, s.cand_n, s.flags};
  if (!ids_a2b) {
    {
      ProfScope prof(VTC_PROF_TOPK, (double)(L2MIN_PLANES + 1) * s.nblk_c * nb * 4, stream);
      launch_minsel(m1, nullptr, stream);
    }
    VTC_LAUNCH_CHECK("minsel");
    return certified_finish(c1, nullptr, stream);
  }
  // both directions: ONE launch per stage (at 10k x 10k a direction alone is 313 minsel workgroups)
  const MinselArgs m2 = minsel_args(s.colk, na, s.nblk_r, RB2, s.nblk_r, nullptr, depth, s.gn, s.gst, s.qmax, kappa, s.cand2, s.cand2_n, s.theta2);
  const Certified c2{{a, b, nb, d, depth, s.flags2, s.colk, na, s.nblk_r, RB2, s.nblk_r, 1, nullptr, s.theta2, ids_a2b, dists_a2b}, s.cand2, s.cand2_n, s.flags2};
  {
    ProfScope prof(VTC_PROF_TOPK, (double)(L2MIN_PLANES + 1) * ((double)s.nblk_c * nb + (double)s.nblk_r * na) * 4, stream);
    launch_minsel(m1, &m2, stream);
  }
  VTC_LAUNCH_CHECK("minsel");
  return certified_finish(c1, &c2, stream);
}
}  // namespace

// ---- sharded sweep: ONE [N/G, N] distance GEMM per rank for both directions (include/vtc_hip.h) ---------------------------
extern "C" int vtc_l2_sweep_shard_supported(int n_total, int n_local, int depth) {
  return exact2_enabled(n_total, n_local, depth) && n_local >= 1 && depth <= n_total;
}

extern "C" size_t vtc_l2_sweep_shard_workspace_bytes(int n_total, int n_local, int d) {
  // rows phase: plan2 of (gallery n_total, queries n_local); cols phase: norms of both sides + candidates of n_local queries
  const size_t rows = plan2(nullptr, n_total, n_local, d, false).total;
  return rows + align_up((size_t)n_total * 4, 256) + 512;
}

extern "C" int vtc_l2_sweep_shard_rows(const float *a_all, const float *b_local, int n_total, int n_local, int d, int depth,
                                       int64_t *ids, float *dists, unsigned *col_planes, int nblk_pad, void *ws, size_t ws_bytes,
                                       void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(a_all && b_local && ids && col_planes && ws, "l2_sweep_shard_rows: null argument");
  VTC_CHECK(d > 0 && d % 64 == 0, "l2_sweep_shard_rows: d=%d must be a positive multiple of 64", d);
  VTC_CHECK(vtc_l2_sweep_shard_supported(n_total, n_local, depth), "l2_sweep_shard_rows: unsupported shape (n_total=%d n_local=%d depth=%d)",
            n_total, n_local, depth);
  Sweep2Ws s2 = plan2((char *)ws, n_total, n_local, d, false);
  VTC_CHECK(nblk_pad >= s2.nblk_r, "l2_sweep_shard_rows: nblk_pad=%d < %d row blocks", nblk_pad, s2.nblk_r);
  VTC_CHECK(ws_bytes >= vtc_l2_sweep_shard_workspace_bytes(n_total, n_local, d), "l2_sweep_shard_rows: workspace too small");
  return exact2_impl(a_all, b_local, n_total, n_local, d, depth, ids, dists, nullptr, nullptr, s2, stream, col_planes, nblk_pad);
}

extern "C" int vtc_l2_sweep_shard_cols(const float *b_all, const float *a_local, int n_total, int n_local, int d, int depth,
                                       const unsigned *planes, int n_src, int nblk_pad, const int *src_base, int64_t *ids,
                                       float *dists, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(b_all && a_local && planes && src_base && ids && ws, "l2_sweep_shard_cols: null argument");
  VTC_CHECK(d > 0 && d % 64 == 0, "l2_sweep_shard_cols: d=%d must be a positive multiple of 64", d);
  VTC_CHECK(vtc_l2_sweep_shard_supported(n_total, n_local, depth) && n_src >= 1 && nblk_pad >= 1,
            "l2_sweep_shard_cols: unsupported shape (n_total=%d n_local=%d depth=%d n_src=%d)", n_total, n_local, depth, n_src);
  VTC_CHECK(ws_bytes >= vtc_l2_sweep_shard_workspace_bytes(n_total, n_local, d), "l2_sweep_shard_cols: workspace too small");
  // gallery = b_all (n_total), queries = a_local (n_local): the plan's qn/gn/cand/flags areas fit as they are
  Sweep2Ws s = plan2((char *)ws, n_total, n_local, d, false);
  sweep_prologue(s, a_local, n_local, b_all, n_total, d, false, stream);
  {
    ProfScope prof(VTC_PROF_TOPK, (double)(L2MIN_PLANES + 1) * n_src * nblk_pad * n_local * 4, stream);
    const MinselArgs m = minsel_args(planes, n_local, n_src * nblk_pad, RB2, nblk_pad, src_base, depth, s.qn, s.qst, s.gmax, exact2_kappa(d), s.cand, s.cand_n, s.theta);
    launch_minsel(m, nullptr, stream);
  }
  VTC_LAUNCH_CHECK("minsel shard cols");
  const Certified c{{a_local, b_all, n_total, d, depth, s.flags, planes, n_local, n_src * nblk_pad, RB2, nblk_pad, n_src, src_base, s.theta, ids, dists}, s.cand, s.cand_n, s.flags};
  return certified_finish(c, nullptr, stream);
}

extern "C" size_t vtc_l2_topk_workspace_bytes(int n_gallery, int n_queries, int d, int precision, int rows_per_block) {
  const size_t v1 = plan(nullptr, n_gallery, n_queries, d, precision, rows_per_block).total;
  if (precision == VTC_SWEEP_EXACT && exact2_enabled(n_gallery, n_queries, 1))
    return std::max(v1, plan2(nullptr, n_gallery, n_queries, d, false).total);     // the depth decides at call time
  return v1;
}

extern "C" int vtc_l2_topk(const float *gallery, const float *queries, int ng, int nq, int d, int depth, int precision,
                           int rows_per_block, int64_t *ids, float *dists, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(ng > 0 && nq > 0 && d > 0, "l2_topk: empty problem");
  VTC_CHECK(depth >= 1 && depth <= 64 && depth <= ng, "l2_topk: depth=%d must be in [1, min(64, n_gallery)]", depth);
  VTC_CHECK(precision >= VTC_SWEEP_F32 && precision <= VTC_SWEEP_EXACT, "l2_topk: bad precision %d", precision);
  VTC_CHECK(d % 64 == 0, "l2_topk: d=%d must be a multiple of 64", d);
  SweepWs s = plan((char *)ws, ng, nq, d, precision, rows_per_block);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_topk: workspace too small (%zu < %zu)", ws_bytes, s.total);
  if (precision != VTC_SWEEP_EXACT) return l2_topk_impl(gallery, queries, ng, nq, d, depth, precision, ids, dists, s, stream);
  if (exact2_enabled(ng, nq, depth) && rows_per_block <= 0) {
    Sweep2Ws s2 = plan2((char *)ws, ng, nq, d, false);
    VTC_CHECK(ws_bytes >= s2.total, "l2_topk: workspace too small (%zu < %zu)", ws_bytes, s2.total);
    return exact2_impl(gallery, queries, ng, nq, d, depth, ids, dists, nullptr, nullptr, s2, stream);
  }
  // EXACT: BF16X3 candidate lists, fp64 re-rank, verified superset property, fp64 brute force for the rest
  const int cdepth = exact_cdepth(depth, ng);
  if (int rc = l2_topk_impl(gallery, queries, ng, nq, d, cdepth, VTC_SWEEP_BF16X3, s.cand, s.cand_d, s, stream)) return rc;
  return exact_finish_lists(gallery, queries, ng, nq, d, depth, cdepth, s.cand, s.cand_d, s.qn, s.gn, s.gmax, s.flags, ids, dists, stream);
}

// Both retrieval directions of RecallAtK (a -> b and b -> a, evaluation/eval.py:117-127) from ONE distance matrix
// D[i][j] = |b_i - a_j|^2: rows give, for every b row, its nearest a rows (ids_b2a: what vtc_l2_topk(gallery = a,
// queries = b) returns); columns give, for every a row, its nearest b rows (ids_a2b = vtc_l2_topk(gallery = b,
// queries = a)).  Same precisions; EXACT re-ranks both candidate sets in fp64.
extern "C" size_t vtc_l2_topk_bidir_workspace_bytes(int n_a, int n_b, int d, int precision, int rows_per_block) {
  const size_t v1 = plan(nullptr, n_a, n_b, d, precision, rows_per_block, true).total;
  if (precision == VTC_SWEEP_EXACT && exact2_enabled(n_a, n_b, 1) && exact2_enabled(n_b, n_a, 1))
    return std::max(v1, plan2(nullptr, n_a, n_b, d, true).total);
  return v1;
}

extern "C" int vtc_l2_topk_bidir(const float *a, const float *b, int n_a, int n_b, int d, int depth, int precision,
                                 int rows_per_block, int64_t *ids_b2a, float *dists_b2a, int64_t *ids_a2b, float *dists_a2b,
                                 void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(n_a > 0 && n_b > 0 && d > 0, "l2_topk_bidir: empty problem");
  VTC_CHECK(depth >= 1 && depth <= 64 && depth <= n_a && depth <= n_b, "l2_topk_bidir: depth=%d must be in [1, min(64, n_a, n_b)]", depth);
  VTC_CHECK(precision >= VTC_SWEEP_F32 && precision <= VTC_SWEEP_EXACT, "l2_topk_bidir: bad precision %d", precision);
  VTC_CHECK(d % 64 == 0, "l2_topk_bidir: d=%d must be a multiple of 64", d);
  VTC_CHECK(ids_b2a && ids_a2b, "l2_topk_bidir: both id outputs are required");
  SweepWs s = plan((char *)ws, n_a, n_b, d, precision, rows_per_block, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_topk_bidir: workspace too small (%zu < %zu)", ws_bytes, s.total);
  if (precision != VTC_SWEEP_EXACT)
    return l2_topk_impl(a, b, n_a, n_b, d, depth, precision, ids_b2a, dists_b2a, s, stream, ids_a2b, dists_a2b);
  if (exact2_enabled(n_a, n_b, depth) && exact2_enabled(n_b, n_a, depth) && rows_per_block <= 0) {
    Sweep2Ws s2 = plan2((char *)ws, n_a, n_b, d, true);
    VTC_CHECK(ws_bytes >= s2.total, "l2_topk_bidir: workspace too small (%zu < %zu)", ws_bytes, s2.total);
    return exact2_impl(a, b, n_a, n_b, d, depth, ids_b2a, dists_b2a, ids_a2b, dists_a2b, s2, stream);
  }
  const int cdepth = std::min(exact_cdepth(depth, n_a), exact_cdepth(depth, n_b));
  if (int rc = l2_topk_impl(a, b, n_a, n_b, d, cdepth, VTC_SWEEP_BF16X3, s.cand, s.cand_d, s, stream, s.cand2, s.cand2_d)) return rc;
  if (int rc = exact_finish_lists(a, b, n_a, n_b, d, depth, cdepth, s.cand, s.cand_d, s.qn, s.gn, s.gmax, s.flags, ids_b2a, dists_b2a, stream)) return rc;
  return exact_finish_lists(b, a, n_b, n_a, d, depth, cdepth, s.cand2, s.cand2_d, s.gn, s.qn, s.qmax, s.flags, ids_a2b, dists_a2b, stream);
}

extern "C" int vtc_recall_hits(const int64_t *ids, int nq, int depth, int64_t target_offset, const int *k_vals, int nk,
                               long long *hits, void *stream) {
  KList kl;
  if (int rc = read_k(kl, "recall_hits", k_vals, nk, depth)) return rc;
  {
    ProfScope prof(VTC_PROF_TOPK, (double)nq * depth * 8, (hipStream_t)stream);
    hipLaunchKernelGGL(recall_hits_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, ids, nq, depth, target_offset,
                       kl.k[0], kl.k[1], kl.k[2], kl.k[3], nk, (unsigned long long *)hits, (const int64_t *)nullptr, (unsigned long long *)nullptr);
  }
  VTC_LAUNCH_CHECK("recall_hits");
  return 0;
}

extern "C" int vtc_recall_hits_pair(const int64_t *ids_a, const int64_t *ids_b, int nq, int depth, int64_t target_offset, const int *k_vals,
                                    int nk, long long *hits_a, long long *hits_b, void *stream) {
  VTC_CHECK(ids_a && ids_b && hits_a && hits_b, "recall_hits_pair: null argument");
  KList kl;
  if (int rc = read_k(kl, "recall_hits_pair", k_vals, nk, depth)) return rc;
  {
    ProfScope prof(VTC_PROF_TOPK, 2.0 * nq * depth * 8, (hipStream_t)stream);
    hipLaunchKernelGGL(recall_hits_kernel, dim3(2 * cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, ids_a, nq, depth, target_offset,
                       kl.k[0], kl.k[1], kl.k[2], kl.k[3], nk, (unsigned long long *)hits_a, ids_b, (unsigned long long *)hits_b);
  }
  VTC_LAUNCH_CHECK("recall_hits_pair");
  return 0;
}
