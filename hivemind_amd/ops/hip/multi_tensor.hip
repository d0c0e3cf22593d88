// Multi-tensor (foreach-style) kernels: one launch covers a whole parameter
// list instead of one kernel per tensor.
//
// Round-1 profiling (profiles/albert_kernels.md) showed 2323 single-tensor
// grad-accumulation adds at 33 us each (6.2% of step) and FusedAdamW
// launching once per parameter. The tensor table
// travels in kernarg space (a by-value struct, ~2.5 KB < the 4 KB limit);
// each thread binary-searches its tensor from the cumulative-offset table
// once per grid-stride chunk -- ~6 compares against a memory-bound body.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#include "multi_tensor.h"

typedef unsigned short ushort_t;

__device__ __forceinline__ int mt_find(const long long* cum, int n, long long i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (i < cum[mid + 1]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ float mt_load_g(const void* g, long long j, bool bf16) {
  if (bf16) return __uint_as_float(((unsigned int)((const ushort_t*)g)[j]) << 16);
  return ((const float*)g)[j];
}

extern "C" __global__ void multi_tensor_adamw(
    MTAdamArgs args, float lr, float beta1, float beta2, float eps,
    float weight_decay, float bias_corr1, float bias_corr2) {
  const long long total = args.cum[args.n];
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int t = mt_find(args.cum, args.n, i);
    long long j = i - args.cum[t];
    float g = mt_load_g(args.g[t], j, (args.g_bf16_mask >> t) & 1);
    float m = args.m[t][j] = beta1 * args.m[t][j] + (1.f - beta1) * g;
    float v = args.v[t][j] = beta2 * args.v[t][j] + (1.f - beta2) * g * g;
    float denom = sqrtf(v / bias_corr2) + eps;
    float p = args.p[t][j];
    p -= lr * (m / bias_corr1 / denom + weight_decay * p);
    args.p[t][j] = p;
    if (args.mirror[t] != nullptr)
      args.mirror[t][j] = __bfloat16_as_ushort(__float2bfloat16(p));
  }
}

extern "C" __global__ void multi_tensor_accumulate(MTAccArgs args, float alpha) {
  const long long total = args.cum[args.n];
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int t = mt_find(args.cum, args.n, i);
    long long j = i - args.cum[t];
    args.acc[t][j] += alpha * mt_load_g(args.x[t], j, (args.x_bf16_mask >> t) & 1);
  }
}

// --------------------------------------------------------------------- LAMB
//
// LAMB needs ||p|| and ||update|| of every tensor before it may touch p, and
// clipping needs the norm of all grads before anything else. Three phases on
// one stream, no float atomics, no host read:
//   grad_sumsq : per-block partial of sum g^2  -> sumsq_finalize -> out[0] += sum
//   stage1     : m, v <- (clip*g); per-block partials of sum p^2, sum u^2
//   trust      : one block per tensor adds its partials in a fixed order
//   stage2     : u recomputed from m, v, p;  p -= lr * trust[t] * u  (+ mirror)
// A block owns chunk c of tensor t (cumblk[] table), so every partial belongs
// to one tensor and the result is bitwise reproducible. Interior elements move
// as 4-element vectors (16 B fp32 / 8 B bf16); the host passes head[t], the
// number of leading elements to peel until all pointers of t are aligned, or
// -1 when they cannot be aligned together.

__device__ __forceinline__ int mt_find_blk(const int* cumblk, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (b < cumblk[mid + 1]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ float mt_bf16_to_f(ushort_t x) {
  return __uint_as_float(((unsigned int)x) << 16);
}

__device__ __forceinline__ float mt_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// sum of (a, b) over the block; valid in thread 0 only. red: one slot per wave.
__device__ __forceinline__ float2 mt_block_sum2(float a, float b, float2* red) {
  a = mt_wave_sum(a);
  b = mt_wave_sum(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = make_float2(a, b);
  __syncthreads();
  float2 r = make_float2(0.f, 0.f);
  if (threadIdx.x == 0) {
    const int waves = blockDim.x >> 6;
    for (int w = 0; w < waves; ++w) { r.x += red[w].x; r.y += red[w].y; }
  }
  return r;
}

// Visit the elements of chunk c of a tensor: one(j) for single elements,
// four(j) for an aligned group j..j+3 that lies fully inside the tensor.
template <class One, class Four>
__device__ __forceinline__ void mt_chunk_walk(long long numel, int head, int c, One&& one,
                                              Four&& four) {
  if (head < 0) {
    const long long lo = (long long)c * MT_LAMB_CHUNK;
    const long long hi = lo + MT_LAMB_CHUNK < numel ? lo + MT_LAMB_CHUNK : numel;
    for (long long j = lo + threadIdx.x; j < hi; j += MT_LAMB_BLOCK) one(j);
    return;
  }
  if (c == 0 && (int)threadIdx.x < head) one((long long)threadIdx.x);  // host keeps head <= numel
  const long long base = head + (long long)c * MT_LAMB_CHUNK;
#pragma unroll
  for (int k = 0; k < MT_LAMB_CHUNK / (4 * MT_LAMB_BLOCK); ++k) {
    const long long j = base + ((long long)k * MT_LAMB_BLOCK + threadIdx.x) * 4;
    if (j + 4 <= numel) {
      four(j);
    } else {
      for (long long e = j; e < numel; ++e) one(e);  // at most 3: the tensor's tail
    }
  }
}

__device__ __forceinline__ void mt_load_g4(const void* g, long long j, bool bf16, float out[4]) {
  if (bf16) {
    const ushort4 r = *reinterpret_cast<const ushort4*>((const ushort_t*)g + j);
    out[0] = mt_bf16_to_f(r.x); out[1] = mt_bf16_to_f(r.y);
    out[2] = mt_bf16_to_f(r.z); out[3] = mt_bf16_to_f(r.w);
  } else {
    const float4 r = *reinterpret_cast<const float4*>((const float*)g + j);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
  }
}

__device__ __forceinline__ float mt_lamb_update(float m, float v, float p, float rbc1, float rbc2,
                                                float eps, float wd) {
  return (m * rbc1) / (sqrtf(v * rbc2) + eps) + wd * p;
}

extern "C" __global__ void __launch_bounds__(MT_LAMB_BLOCK)
multi_tensor_grad_sumsq(MTSumsqArgs args, float* __restrict__ partials) {
  __shared__ float2 red[MT_LAMB_BLOCK / 64];
  const int t = __builtin_amdgcn_readfirstlane(mt_find_blk(args.cumblk, args.n, blockIdx.x));
  const int c = blockIdx.x - args.cumblk[t];
  const void* g = args.g[t];
  const bool bf16 = (args.g_bf16_mask >> t) & 1;
  float acc = 0.f;
  mt_chunk_walk(
      args.numel[t], args.head[t], c,
      [&](long long j) { float x = mt_load_g(g, j, bf16); acc += x * x; },
      [&](long long j) {
        float x[4];
        mt_load_g4(g, j, bf16, x);
        acc += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
      });
  const float2 r = mt_block_sum2(acc, 0.f, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = r.x;
}

// out[0] += sum(partials): one block, thread-strided then tree -- fixed order
extern "C" __global__ void __launch_bounds__(1024)
mt_sumsq_finalize(const float* __restrict__ partials, long long count, float* out) {
  __shared__ float2 red[1024 / 64];
  float acc = 0.f;
  for (long long i = threadIdx.x; i < count; i += 1024) acc += partials[i];
  const float2 r = mt_block_sum2(acc, 0.f, red);
  if (threadIdx.x == 0) out[0] += r.x;
}

extern "C" __global__ void __launch_bounds__(MT_LAMB_BLOCK)
multi_tensor_lamb_stage1(MTLambArgs args, float beta1, float beta2, float omb1, float omb2,
                         float eps, float wd,
                         float rbc1, float rbc2, const float* __restrict__ clip_ptr,
                         float2* __restrict__ partials) {
  __shared__ float2 red[MT_LAMB_BLOCK / 64];
  const int t = __builtin_amdgcn_readfirstlane(mt_find_blk(args.cumblk, args.n, blockIdx.x));
  const int c = blockIdx.x - args.cumblk[t];
  const float* __restrict__ p = args.p[t];
  const void* __restrict__ g = args.g[t];
  float* __restrict__ m = args.m[t];
  float* __restrict__ v = args.v[t];
  const bool bf16 = (args.g_bf16_mask >> t) & 1;
  const float clip = clip_ptr != nullptr ? clip_ptr[0] : 1.f;
  float sp = 0.f, su = 0.f;
  mt_chunk_walk(
      args.numel[t], args.head[t], c,
      [&](long long j) {
        const float gj = clip * mt_load_g(g, j, bf16);
        const float pj = p[j];
        const float mj = beta1 * m[j] + omb1 * gj;
        const float vj = beta2 * v[j] + omb2 * gj * gj;
        m[j] = mj;
        v[j] = vj;
        const float u = mt_lamb_update(mj, vj, pj, rbc1, rbc2, eps, wd);
        sp += pj * pj;
        su += u * u;
      },
      [&](long long j) {
        float gq[4];
        mt_load_g4(g, j, bf16, gq);
        const float4 pq = *reinterpret_cast<const float4*>(p + j);
        float4 mq = *reinterpret_cast<const float4*>(m + j);
        float4 vq = *reinterpret_cast<const float4*>(v + j);
        const float pa[4] = {pq.x, pq.y, pq.z, pq.w};
        float ma[4] = {mq.x, mq.y, mq.z, mq.w};
        float va[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ge = clip * gq[e];
          ma[e] = beta1 * ma[e] + omb1 * ge;
          va[e] = beta2 * va[e] + omb2 * ge * ge;
          const float u = mt_lamb_update(ma[e], va[e], pa[e], rbc1, rbc2, eps, wd);
          sp += pa[e] * pa[e];
          su += u * u;
        }
        *reinterpret_cast<float4*>(m + j) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *reinterpret_cast<float4*>(v + j) = make_float4(va[0], va[1], va[2], va[3]);
      });
  const float2 r = mt_block_sum2(sp, su, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// one block per tensor: trust[t] = clamp(||p|| / ||u||, lo, hi), 1 if either norm is 0
extern "C" __global__ void __launch_bounds__(MT_LAMB_BLOCK)
multi_tensor_lamb_trust(MTLambArgs args, const float2* __restrict__ partials,
                        float* __restrict__ trust, float trust_lo, float trust_hi) {
  __shared__ float2 red[MT_LAMB_BLOCK / 64];
  const int t = blockIdx.x;
  const int b0 = args.cumblk[t], b1 = args.cumblk[t + 1];
  float sp = 0.f, su = 0.f;
  for (int i = b0 + threadIdx.x; i < b1; i += MT_LAMB_BLOCK) {
    const float2 x = partials[i];
    sp += x.x;
    su += x.y;
  }
  const float2 r = mt_block_sum2(sp, su, red);
  if (threadIdx.x == 0) {
    const float p_norm = sqrtf(r.x), u_norm = sqrtf(r.y);
    float ratio = (p_norm > 0.f && u_norm > 0.f) ? p_norm / u_norm : 1.f;
    trust[t] = fminf(fmaxf(ratio, trust_lo), trust_hi);
  }
}

extern "C" __global__ void __launch_bounds__(MT_LAMB_BLOCK)
multi_tensor_lamb_stage2(MTLambArgs args, float lr, float eps, float wd, float rbc1, float rbc2,
                         const float* __restrict__ trust) {
  const int t = __builtin_amdgcn_readfirstlane(mt_find_blk(args.cumblk, args.n, blockIdx.x));
  const int c = blockIdx.x - args.cumblk[t];
  float* __restrict__ p = args.p[t];
  const float* __restrict__ m = args.m[t];
  const float* __restrict__ v = args.v[t];
  mt_ushort* __restrict__ mirror = args.mirror[t];
  const float scale = lr * trust[t];
  mt_chunk_walk(
      args.numel[t], args.head[t], c,
      [&](long long j) {
        float pj = p[j];
        pj -= scale * mt_lamb_update(m[j], v[j], pj, rbc1, rbc2, eps, wd);
        p[j] = pj;
        if (mirror != nullptr) mirror[j] = __bfloat16_as_ushort(__float2bfloat16(pj));
      },
      [&](long long j) {
        const float4 pq = *reinterpret_cast<const float4*>(p + j);
        const float4 mq = *reinterpret_cast<const float4*>(m + j);
        const float4 vq = *reinterpret_cast<const float4*>(v + j);
        float pa[4] = {pq.x, pq.y, pq.z, pq.w};
        const float ma[4] = {mq.x, mq.y, mq.z, mq.w};
        const float va[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pa[e] -= scale * mt_lamb_update(ma[e], va[e], pa[e], rbc1, rbc2, eps, wd);
        *reinterpret_cast<float4*>(p + j) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        if (mirror != nullptr) {
          ushort4 o;
          o.x = __bfloat16_as_ushort(__float2bfloat16(pa[0]));
          o.y = __bfloat16_as_ushort(__float2bfloat16(pa[1]));
          o.z = __bfloat16_as_ushort(__float2bfloat16(pa[2]));
          o.w = __bfloat16_as_ushort(__float2bfloat16(pa[3]));
          *reinterpret_cast<ushort4*>(mirror + j) = o;
        }
      });
}

extern "C" void launch_multi_tensor_lamb(const MTLambArgs* args, float lr, double beta1, double beta2,
                                         float eps, float weight_decay, double bias_corr1,
                                         double bias_corr2, float trust_lo, float trust_hi,
                                         const float* clip, float* partials, float* trust,
                                         void* stream) {
  const int blocks = args->cumblk[args->n];
  const float rbc1 = (float)(1.0 / bias_corr1), rbc2 = (float)(1.0 / bias_corr2);
  hipStream_t s = (hipStream_t)stream;
  if (args->n < 1) return;
  if (blocks > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_stage1, dim3(blocks), dim3(MT_LAMB_BLOCK), 0, s, *args,
                       (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps,
                       weight_decay, rbc1, rbc2, clip, (float2*)partials);
  hipLaunchKernelGGL(multi_tensor_lamb_trust, dim3(args->n), dim3(MT_LAMB_BLOCK), 0, s, *args,
                     (const float2*)partials, trust, trust_lo, trust_hi);
  if (blocks > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_stage2, dim3(blocks), dim3(MT_LAMB_BLOCK), 0, s, *args,
                       lr, eps, weight_decay, rbc1, rbc2, (const float*)trust);
}

extern "C" void launch_multi_tensor_grad_sumsq(const MTSumsqArgs* args, float* partials,
                                               void* stream) {
  const int blocks = args->cumblk[args->n];
  if (blocks > 0)
    hipLaunchKernelGGL(multi_tensor_grad_sumsq, dim3(blocks), dim3(MT_LAMB_BLOCK), 0,
                       (hipStream_t)stream, *args, partials);
}

extern "C" void launch_sumsq_finalize(const float* partials, long long count, float* out,
                                      void* stream) {
  hipLaunchKernelGGL(mt_sumsq_finalize, dim3(1), dim3(1024), 0, (hipStream_t)stream, partials,
                     count, out);
}

extern "C" void launch_multi_tensor_adamw(const MTAdamArgs* args, float lr, float beta1,
                                          float beta2, float eps, float weight_decay,
                                          float bias_corr1, float bias_corr2, void* stream) {
  long long total = args->cum[args->n];
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(multi_tensor_adamw, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                     *args, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2);
}

extern "C" void launch_multi_tensor_accumulate(const MTAccArgs* args, float alpha, void* stream) {
  long long total = args->cum[args->n];
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(multi_tensor_accumulate, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, *args, alpha);
}
