// audio.hip -- the audio branch's feature MLP (model/model.py:80-94 `MLP`, applied per clip at :220-230), eval mode, ONE launch:
//     y = W2 relu(W1' x + b1') + b2          x, y: [n, 512] fp32
// W1', b1' are Linear(512, 512) with BatchNorm1d's running statistics folded in on the host (vtc_amd/towers.py PackedAudioMlp, fp64);
// Dropout is the identity in eval mode.  Rows are the clips of a batch in [B * na, 512] order, which is the row layout the CAM reads
// its aux tokens from (vtc_cam_forward_aux), so the output goes there directly.
//
// Work split: a workgroup owns a 16-row tile (one fp32 MFMA tile, v_mfma_f32_16x16x4_f32: exact fp32, k order permuted identically
// for both operands as in cam.hip) and a 1/S share of the hidden layer.  It stages the x tile in LDS, computes its hidden columns
// (W1' rows streamed from L2 as the A operand), keeps them in LDS after bias + ReLU, and multiplies them by the matching K-slice of W2.
//   S = 1 (many tiles: n >= ~2 K rows): the result is stored as is; every workgroup reads the full 2 MB of weights from L2.
//   S > 1 (few tiles: the weights are the cost): each workgroup reads 2 MB / S, stores its [16, 512] partial write-through (sc1),
//   draws a ticket from the tile's counter, and the last arriver sums the S partials in split order (bitwise reproducible) and
//   stores y.  Counters are zeroed by a hipMemsetAsync in front of the launch.
#include "common.h"

namespace {

constexpr int MLP_D = 512;                  // MLP(num_features = 512, num_classes = 512): the only width the reference builds
constexpr int MLP_LD = MLP_D + 4;           // padded LDS row (floats)
constexpr int MLP_MAX_SPLIT = 8;

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

// write-through / L1-bypassing accesses (aux 16 = sc1) to the partial slabs one workgroup hands to another
struct Sc1Slab {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ Sc1Slab(const void *base, size_t bytes) {
    r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)(bytes < 0xFFFFFFF0u ? bytes : 0xFFFFFFF0u), 0x00020000);
  }
  __device__ __forceinline__ float4 ld16(int off) const {
    const v4u_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
  __device__ __forceinline__ void st16(int off, float4 v) const {
    const v4u_t vv = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(vv, r, off, 0, 16);
  }
};

// torch.relu: a NaN stays NaN (fmaxf(NaN, 0) would return 0 and hide a non-finite input from the watchdog)
__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }

// acc[16 x 16] += W[n0 + i][k0 + k] * A[j][k], k in [0, K): W row-major with leading dimension ldw (global), A: LDS rows of MLP_LD floats.
// Lane (g, m) holds W[n0 + m][k0 + 16 q + 4 g ..] and A[m][16 q + 4 g ..]: the result lane (g, m) holds out column n0 + 4 g + v of row m.
template <int K>
__device__ __forceinline__ f32x4 tile_mfma(const float *__restrict__ W, int ldw, int n0, int k0, const float *A, int lane) {
  const int g = lane >> 4, m = lane & 15;
  const float *wrow = W + (size_t)(n0 + m) * ldw + k0 + 4 * g;
  const float *arow = A + m * MLP_LD + 4 * g;
  float4 wv[K / 16];                    // the whole weight slice in flight at once: one memory latency per slice
#pragma unroll
  for (int q = 0; q < K / 16; ++q) wv[q] = *reinterpret_cast<const float4 *>(wrow + 16 * q);
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;        // four independent chains (40-cycle dependent latency)
#pragma unroll
  for (int q = 0; q < K / 16; ++q) {
    const float4 xv = *reinterpret_cast<const float4 *>(arow + 16 * q);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q].x, xv.x, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q].y, xv.y, a1, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q].z, xv.z, a2, 0, 0, 0);
    a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[q].w, xv.w, a3, 0, 0, 0);
  }
  return (a0 + a1) + (a2 + a3);
}

// grid (tiles, S), 256 threads.  HC = MLP_D / S hidden columns per workgroup.
template <int HC>
__global__ __launch_bounds__(256, 2) void feature_mlp_kernel(const float *__restrict__ x, int n, const float *__restrict__ w1,
                                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                                             const float *__restrict__ b2, float *__restrict__ y, float *__restrict__ slab,
                                                             int *__restrict__ cnt) {
  constexpr int S = MLP_D / HC;
  __shared__ __attribute__((aligned(16))) float lds[2 * 16 * MLP_LD + 4];     // x tile, hidden tile, the "last arriver" word
  float *xs = lds, *hs = lds + 16 * MLP_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, m = lane & 15;
  const int tile = blockIdx.x, sp = blockIdx.y, row0 = 16 * tile;
  // x tile -> LDS (rows past n repeat row n - 1: computed, never stored)
#pragma unroll
  for (int i = 0; i < 16 * MLP_D / 4 / 256; ++i) {
    const int e = tid + 256 * i, r = e / (MLP_D / 4), c = 4 * (e % (MLP_D / 4));
    *reinterpret_cast<float4 *>(xs + r * MLP_LD + c) = *reinterpret_cast<const float4 *>(x + (size_t)min(row0 + r, n - 1) * MLP_D + c);
  }
  __syncthreads();
  // hidden columns [sp HC, (sp + 1) HC): HC / 64 slices of 16 per wave; bias + ReLU; kept in LDS (local column index)
#pragma unroll 1
  for (int j = 0; j < HC / 64; ++j) {
    const int lc = 16 * (wave * (HC / 64) + j), hc = sp * HC + lc;
    const f32x4 acc = tile_mfma<MLP_D>(w1, MLP_D, hc, 0, xs, lane);
    const float4 bb = *reinterpret_cast<const float4 *>(b1 + hc + 4 * g);
    *reinterpret_cast<float4 *>(hs + m * MLP_LD + lc + 4 * g) = make_float4(relu(acc[0] + bb.x), relu(acc[1] + bb.y), relu(acc[2] + bb.z), relu(acc[3] + bb.w));
  }
  __syncthreads();
  // output columns: 8 slices of 16 per wave, K = this workgroup's HC hidden columns
  const Sc1Slab part(slab, (size_t)gridDim.x * S * 16 * MLP_D * 4);
#pragma unroll 1
  for (int j = 0; j < MLP_D / 64; ++j) {
    const int oc = 16 * (wave * (MLP_D / 64) + j);
    const f32x4 acc = tile_mfma<HC>(w2, MLP_D, oc, sp * HC, hs, lane);
    if constexpr (S == 1) {
      const int r = row0 + m;
      if (r < n) {
        const float4 bb = *reinterpret_cast<const float4 *>(b2 + oc + 4 * g);
        *reinterpret_cast<float4 *>(y + (size_t)r * MLP_D + oc + 4 * g) = make_float4(acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w);
      }
    } else {
      part.st16((((tile * S + sp) * 16 + m) * MLP_D + oc + 4 * g) * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
  }
  if constexpr (S > 1) {
    // hand-off of the partials: write-through stores drained by every wave, one relaxed agent-scope ticket; the last arriver reads
    // every slab with sc1 loads (no fences needed in this form)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int *last = reinterpret_cast<int *>(lds + 2 * 16 * MLP_LD);
    if (tid == 0) *last = __hip_atomic_fetch_add(cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S - 1;
    __syncthreads();
    if (!*last) return;
#pragma unroll
    for (int i = 0; i < 16 * MLP_D / 4 / 256; ++i) {
      const int e = tid + 256 * i, r = e / (MLP_D / 4), c = 4 * (e % (MLP_D / 4));
      if (row0 + r >= n) continue;
      float4 s = part.ld16((((tile * S) * 16 + r) * MLP_D + c) * 4);
#pragma unroll
      for (int k = 1; k < S; ++k) {
        const float4 v = part.ld16((((tile * S + k) * 16 + r) * MLP_D + c) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      const float4 bb = *reinterpret_cast<const float4 *>(b2 + c);
      *reinterpret_cast<float4 *>(y + (size_t)(row0 + r) * MLP_D + c) = make_float4(s.x + bb.x, s.y + bb.y, s.z + bb.z, s.w + bb.w);
    }
  }
}

}  // namespace

// hidden split: grow S while the grid stays within half the CUs (the weights, not the rows, are the cost at small n)
static int mlp_split(int n) {
  const int tiles = cdiv(n, 16);
  int s = 1;
  while (s < MLP_MAX_SPLIT && tiles * s * 2 <= vtcgemm::num_cus()) s *= 2;
  return s;
}

extern "C" size_t vtc_feature_mlp_workspace_bytes(int n, int d) {
  if (n <= 0 || d != MLP_D) return 0;
  const int s = mlp_split(n), tiles = cdiv(n, 16);
  if (s == 1) return 0;
  return align_up((size_t)tiles * s * 16 * MLP_D * 4, 256) + align_up((size_t)tiles * 4, 256);
}

extern "C" int vtc_feature_mlp(const float *x, int n, int d, const float *w1, const float *b1, const float *w2, const float *b2, float *y,
                               void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t s = (hipStream_t)stream_;
  VTC_CHECK(x && w1 && b1 && w2 && b2 && y, "feature_mlp: null argument");
  VTC_CHECK(d == MLP_D, "feature_mlp: width %d (the audio MLP is 512 x 512)", d);
  VTC_CHECK(n > 0, "feature_mlp: n=%d", n);
  const size_t need = vtc_feature_mlp_workspace_bytes(n, d);
  VTC_CHECK(ws_bytes >= need && (ws || need == 0), "feature_mlp: workspace too small (%zu < %zu)", ws_bytes, need);
  const int split = mlp_split(n), tiles = cdiv(n, 16);
  float *slab = (float *)ws;
  int *cnt = split > 1 ? (int *)((char *)ws + align_up((size_t)tiles * split * 16 * MLP_D * 4, 256)) : nullptr;
  if (split > 1) VTC_CHECK(hipMemsetAsync(cnt, 0, (size_t)tiles * 4, s) == hipSuccess, "feature_mlp: counter reset failed");
  ProfScope prof(VTC_PROF_GEMM_F32, 4.0 * n * MLP_D * MLP_D, s);
  const dim3 grid(tiles, split);
  switch (split) {
    case 1: hipLaunchKernelGGL(feature_mlp_kernel<512>, grid, dim3(256), 0, s, x, n, w1, b1, w2, b2, y, slab, cnt); break;
    case 2: hipLaunchKernelGGL(feature_mlp_kernel<256>, grid, dim3(256), 0, s, x, n, w1, b1, w2, b2, y, slab, cnt); break;
    case 4: hipLaunchKernelGGL(feature_mlp_kernel<128>, grid, dim3(256), 0, s, x, n, w1, b1, w2, b2, y, slab, cnt); break;
    default: hipLaunchKernelGGL(feature_mlp_kernel<64>, grid, dim3(256), 0, s, x, n, w1, b1, w2, b2, y, slab, cnt); break;
  }
  VTC_LAUNCH_CHECK("feature_mlp");
  return 0;
}
