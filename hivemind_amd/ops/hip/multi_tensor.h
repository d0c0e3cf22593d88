// Shared host/device declarations for the multi-tensor kernels.
#pragma once
#include <cstdint>

#define MT_CHUNK 48

typedef unsigned short mt_ushort;

struct MTAdamArgs {
  float* p[MT_CHUNK];
  const void* g[MT_CHUNK];
  float* m[MT_CHUNK];
  float* v[MT_CHUNK];
  mt_ushort* mirror[MT_CHUNK];
  long long cum[MT_CHUNK + 1];
  int n;
  unsigned long long g_bf16_mask;
};

struct MTAccArgs {
  float* acc[MT_CHUNK];
  const void* x[MT_CHUNK];
  long long cum[MT_CHUNK + 1];
  int n;
  unsigned long long x_bf16_mask;
};

// LAMB / grad-norm kernels: every block owns one fixed-size chunk of ONE
// tensor (cumblk[] is the cumulative chunk table), so each per-block partial
// sum belongs to exactly one tensor and the final sums run in a fixed order.
#define MT_LAMB_BLOCK 256
#define MT_LAMB_CHUNK 4096  // elements per block: 256 threads x 4 groups of 4

// head[t] >= 0: the first head[t] elements are handled one by one, after which
// every pointer of tensor t is aligned for 4-element vector access (16 B for
// fp32, 8 B for bf16). head[t] < 0: the pointers of tensor t cannot be aligned
// together, the whole tensor takes the scalar path.
struct MTLambArgs {
  float* p[MT_CHUNK];
  const void* g[MT_CHUNK];
  float* m[MT_CHUNK];
  float* v[MT_CHUNK];
  mt_ushort* mirror[MT_CHUNK];
  long long numel[MT_CHUNK];
  int cumblk[MT_CHUNK + 1];
  int head[MT_CHUNK];
  int n;
  unsigned long long g_bf16_mask;
};

struct MTSumsqArgs {
  const void* g[MT_CHUNK];
  long long numel[MT_CHUNK];
  int cumblk[MT_CHUNK + 1];
  int head[MT_CHUNK];
  int n;
  unsigned long long g_bf16_mask;
};

// partials: float2 {sum p^2, sum u^2} per block of this launch; trust: float per tensor
// betas and bias corrections arrive in double: 1 - beta and 1 / bias_corr are
// rounded to fp32 once, not computed from already rounded fp32 values
extern "C" void launch_multi_tensor_lamb(const MTLambArgs*, float lr, double beta1, double beta2,
                                         float eps, float weight_decay, double bias_corr1,
                                         double bias_corr2, float trust_lo, float trust_hi,
                                         const float* clip, float* partials, float* trust,
                                         void* stream);
// partials: one float per block of this launch
extern "C" void launch_multi_tensor_grad_sumsq(const MTSumsqArgs*, float* partials, void* stream);
// out[0] += sum(partials[0..count)) in a fixed order
extern "C" void launch_sumsq_finalize(const float* partials, long long count, float* out,
                                      void* stream);

extern "C" void launch_multi_tensor_adamw(const MTAdamArgs*, float, float, float, float,
                                          float, float, float, void*);
extern "C" void launch_multi_tensor_accumulate(const MTAccArgs*, float, void*);
