// loss.hip -- the batch-level similarity and the CLIP loss.
//   vtc_similarity  exp(logit_scale) * V @ T^T (model/model.py:369,478,504,621)
//   vtc_clip_loss   0.5 (CE(sim, arange) + CE(sim^T, arange)) (model/loss.py:18-22)
#include "common.h"

namespace {

// terms[i] = lse(sim[i,:]) - sim[i,i];  terms[n + j] = lse(sim[:,j]) - sim[j,j]
__global__ __launch_bounds__(256) void lse_terms_kernel(const float *__restrict__ sim, int n, float *__restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= 2 * n) return;
  const bool col = w >= n;
  const int i = col ? w - n : w;
  const size_t stride = col ? (size_t)n : 1, base = col ? (size_t)i : (size_t)i * n;
  float mx = -INFINITY;
  for (int c = lane; c < n; c += 64) mx = fmaxf(mx, sim[base + c * stride]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int c = lane; c < n; c += 64) s += expf(sim[base + c * stride] - mx);
  s = wave_sum(s);
  if (lane == 0) terms[w] = mx + logf(s) - sim[(size_t)i * n + i];
}

__global__ __launch_bounds__(256) void loss_reduce_kernel(const float *__restrict__ terms, int n, float *__restrict__ loss) {
  __shared__ float part[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < 2 * n; i += 256) s += terms[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = 0.5f * ((part[0] + part[1]) + (part[2] + part[3])) / n;
}
}  // namespace

extern "C" int vtc_similarity(const float *v, const float *t, int nv, int nt, int d, const float *logit_scale, float *sim,
                              void *stream) {
  GemmEpi e;
  e.mode = EPI_SCALE; e.out_dtype = VTC_F32; e.scale_log = logit_scale;
  return launch_gemm(v, t, nullptr, sim, nv, nt, d, VTC_F32, e, (hipStream_t)stream);
}

extern "C" size_t vtc_clip_loss_workspace_bytes(int n) { return (size_t)2 * n * sizeof(float); }

extern "C" int vtc_clip_loss(const float *sim, int n, float *loss, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(n > 0, "clip_loss: n=%d", n);
  VTC_CHECK(ws && ws_bytes >= vtc_clip_loss_workspace_bytes(n), "clip_loss: workspace too small");
  hipLaunchKernelGGL(lse_terms_kernel, dim3(cdiv(2 * n, 4)), dim3(256), 0, stream, sim, n, (float *)ws);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, stream, (const float *)ws, n, loss);
  VTC_LAUNCH_CHECK("clip_loss");
  return 0;
}
