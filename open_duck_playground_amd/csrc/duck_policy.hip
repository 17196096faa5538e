// The deterministic policy of the evaluator in one launch (include/duck_ppo.h: duck_policy_act): brax's
// policy MLP (ppo/networks.py: Dense layers with swish between them) and NormalTanhDistribution.mode,
// obs -> normaliser -> every layer -> logits, tanh(loc). The rollout's chain runs one duck_mlp_gemm launch
// per layer (csrc/duck_mlp.hip) with the hidden activations in global memory; here a 256-thread workgroup
// takes 16 rows through all layers and the activations never leave LDS.
//
// Bit identity with that chain. An output element of gemm_tile is one v_mfma_f32_16x16x4_f32 chain over
// ascending k-steps from a zero accumulator -- lane group lk feeds reduction index 4 s + lk of k-step s, the
// reduction zero-padded to a multiple of 32 -- then + bias, then silu through sigm / __expf. None of that
// depends on the tile shape, and this kernel feeds its MFMAs the same operands in the same order, so the
// logits equal the chain's bit for bit (tests/test_gpu_evaluator.py compares them as integers).
//
// LDS. Two activation buffers (layer l reads buffer l & 1 and writes the other), each a row of 32-deep
// reduction chunks in duck_mlp.hip's swizzled [row][lk][s] image, 16 rows x 32 words per chunk: a lane's 8
// k-steps of a chunk are two ds_read_b128, conflict-free. The weights stream from L2 in
// tiles of 128 output columns x 32 reduction indices through two LDS buffers of the same image (wave w
// owns columns 32 w .. 32 w + 31 of the tile: 2 MFMA tiles); a tile's global loads are issued two
// tiles ahead into registers and stored one tile ahead, one barrier per tile, the sequence running
// through the column groups of a layer without draining.
//
// Several policies in one launch (duck_policy_act_multi). An MFMA tile shares one weight operand across its 16
// rows, so a policy per row becomes a policy per tile: rows seg[k] .. seg[k + 1] - 1 belong to policy k, and a
// workgroup takes up to 16 consecutive rows of ONE segment through policy_tile. Only the weight, bias and
// normaliser bases and the row bounds depend on k, so a row's bits are those of duck_policy_act with policy k's
// parameters alone. The block index maps to (policy, tile) through by-value tables (MultiArgs) in one of two
// orders, DESIGN.md §9 "Policies". There is one kernel: duck_policy_act is K = 1 with the segment [0, N) in the
// policy-major order, where block b takes tile b as it always did.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "duck_common.h"
#include "../../include/duck_ppo.h"

namespace {

constexpr int KC = 32;    // reduction chunk (as duck_mlp.hip: the zero padding of the reduction is part of the bits)
constexpr int TR = 16;    // rows per workgroup (one MFMA tile high)
constexpr int CG = 128;   // output columns per weight tile (4 waves x 2 MFMA tiles)
constexpr int MAXW = 512; // widest layer
constexpr int BS_WORDS = CG * KC;
using f4 = __attribute__((ext_vector_type(4))) float;

// duck_mlp.hip's image of a [row][32] chunk: word (row, k) at [row][k & 3][k >> 2], the 4-word blocks of row r
// XOR-swizzled by (2 r + (r >> 3)) & 7 (r mod 16)
__device__ __forceinline__ int swz_word(int row, int k) {
  const int kp = (k & 3) * 8 + (k >> 2), r = row & 15;
  return row * KC + ((((kp >> 2) ^ ((2 * r + (r >> 3)) & 7))) << 2) + (kp & 3);
}
// k-steps 4 h .. 4 h + 3 of lane group lk in row x of a chunk image
__device__ __forceinline__ f4 chunk_ksteps(const float* S, int x, int lk, int h) {
  const int r = x & 15, f = (2 * r + (r >> 3)) & 7;
  return *(const f4*)(S + x * KC + (((2 * lk + h) ^ f) << 2));
}
__device__ __forceinline__ int act_word(int row, int k) { return (k >> 5) * (TR * KC) + swz_word(row, k & 31); }

__device__ __forceinline__ float sigm(float z) { return 1.f / (1.f + __expf(-z)); }

struct PolicyArgs {
  int N, nl;
  int sizes[DUCK_POLICY_MAX_LAYERS + 1];
  const float* W[DUCK_POLICY_MAX_LAYERS];
  const float* b[DUCK_POLICY_MAX_LAYERS];
  const float *mean, *istd, *obs;
  float *logits, *action;
  int buf_words[2];  // LDS words of the two activation buffers
};

// one weight tile in registers: thread t holds reduction indices 4 (t & 7) .. + 3 of tile rows (output columns)
// (t >> 3) + 32 p, zeros past the layer's outputs and past its inputs
struct WTile {
  float v[16];
  __device__ void load(const float* __restrict__ W, int R, int M, int c0, int k0) {
    const int k = k0 + 4 * ((int)threadIdx.x & 7);
    const bool vec = ((R & 3) == 0) && (((size_t)W & 15) == 0) && k + 4 <= R;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int col = c0 + ((int)threadIdx.x >> 3) + 32 * p;
      const bool ok = col < M;
      const float* row = W + (size_t)(ok ? col : 0) * R;
      if (vec) {
        const f4 x = ok ? *(const f4*)(row + k) : f4{0.f, 0.f, 0.f, 0.f};
        v[4 * p] = x[0]; v[4 * p + 1] = x[1]; v[4 * p + 2] = x[2]; v[4 * p + 3] = x[3];
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[4 * p + q] = (ok && k + q < R) ? row[k + q] : 0.f;
      }
    }
  }
  __device__ void store(float* S) const {
    const int c = 4 * ((int)threadIdx.x & 7);
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int r = ((int)threadIdx.x >> 3) + 32 * p;
#pragma unroll
      for (int q = 0; q < 4; q++) S[swz_word(r, c + q)] = v[4 * p + q];
    }
  }
};

// Rows r0 .. r0 + 15 below N through every layer of policy k (the parameters of policy k lie k layers' worth
// behind a.W[l], a.b[l], a.mean, a.istd; N: the end of the policy's segment)
__device__ __forceinline__ void policy_tile(const PolicyArgs& a, const int r0, const int N, const int k) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Bs = smem;  // two weight tiles
  float* const act0 = smem + 2 * BS_WORDS;
  float* const act1 = act0 + a.buf_words[0];
  const int tid = threadIdx.x, l = tid & 63, li = l & 15, lk = l >> 4, w = tid >> 6;

  // the observation rows, normalised as duck_mlp_gemm's loads normalise them, into buffer 0
  {
    const int R = a.sizes[0], Rp = (R + KC - 1) / KC * KC;
    const float* mean = a.mean ? a.mean + (size_t)k * R : nullptr;
    const float* istd = a.mean ? a.istd + (size_t)k * R : nullptr;
    for (int i = tid; i < TR * Rp; i += 256) {
      const int row = i / Rp, c = i - row * Rp;
      const bool ok = r0 + row < N && c < R;
      float x = ok ? a.obs[(size_t)(r0 + row) * R + c] : 0.f;
      if (mean && ok) x = (x - mean[c]) * istd[c];
      act0[act_word(row, c)] = x;
    }
  }

  for (int layer = 0; layer < a.nl; layer++) {
    const int R = a.sizes[layer], M = a.sizes[layer + 1];
    const float* __restrict__ W = a.W[layer] + (size_t)k * M * R;
    const float* __restrict__ bias = a.b[layer] + (size_t)k * M;
    const float* in = (layer & 1) ? act1 : act0;
    float* out = (layer & 1) ? act0 : act1;
    const bool last = layer == a.nl - 1;
    const int nch = (R + KC - 1) / KC, ncg = (M + CG - 1) / CG, nit = nch * ncg;
    const int Mp = (M + KC - 1) / KC * KC;  // the next layer's padded reduction
    WTile wt[2];  // set i & 1 holds tile i = (column group i / nch, chunk i % nch)
    auto load = [&](auto S, int it) {
      const int cg = it / nch;
      wt[decltype(S)::value].load(W, R, M, cg * CG, (it - cg * nch) * KC);
    };
    f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
    const std::integral_constant<int, 0> S0;
    const std::integral_constant<int, 1> S1;
    load(S0, 0);
    if (nit > 1) load(S1, 1);
    wt[0].store(Bs);
    __syncthreads();  // (also: the layer's input, written by the loop above or the previous layer's epilogues)
    auto body = [&](int it, auto S, auto SN) {
      constexpr int s = decltype(S)::value, sn = decltype(SN)::value;
      const int cg = it / nch, c = it - cg * nch;
      if (it + 2 < nit) load(S, it + 2);  // set s held tile it, already in LDS
      const float* As = in + c * (TR * KC);
      const float* Bt = Bs + s * BS_WORDS;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const f4 av = chunk_ksteps(As, li, lk, h);
        f4 bv[2];
#pragma unroll
        for (int j = 0; j < 2; j++) bv[j] = chunk_ksteps(Bt, 32 * w + 16 * j + li, lk, h);
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[j][q], acc[j], 0, 0, 0);
      }
      if (it + 1 < nit) wt[sn].store(Bs + sn * BS_WORDS);  // read last in tile it - 1, before the barrier
      if (c == nch - 1) {
        // acc[j][q] is C[4 lk + q][cg CG + 32 w + 16 j + li]
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int col = cg * CG + 32 * w + 16 * j + li;
          const float bj = col < M ? bias[col] : 0.f;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int row = 4 * lk + q;
            const bool ok = r0 + row < N && col < M;
            const float z = acc[j][q] + bj;
            if (last) {
              if (ok) {
                if (a.logits) a.logits[(size_t)(r0 + row) * M + col] = z;
                if (col < M / 2) a.action[(size_t)(r0 + row) * (M / 2) + col] = tanhf(z);
              }
            } else if (col < Mp) {  // rows past N and the reduction's padding feed zeros
              out[act_word(row, col)] = ok ? z * sigm(z) : 0.f;
            }
          }
          acc[j] = f4{0.f, 0.f, 0.f, 0.f};
        }
      }
      __syncthreads();
    };
    for (int it = 0; it < nit; it += 2) {
      body(it, S0, S1);
      if (it + 1 < nit) body(it + 1, S1, S0);
    }
  }
}

// Block index -> (policy, tile of the policy's segment), tables by value. nt(k) = ceil((seg[k+1] - seg[k]) / 16).
//   order 0, policy-major: policy k's tiles are blocks start[k] .. start[k] + nt(k) - 1, start the running sum.
//   order 1, dealt over the XCDs: blocks b and b + 8 have been observed on one XCD, so "lane" b & 7 stands for an
//     XCD and b >> 3 is a position in it. K >= 8: policy k's tiles are positions start[k] .. + nt(k) - 1 of lane
//     k & 7 (start the running sum over the lane's policies k & 7, k & 7 + 8, ...): one L2 sees the weights of K / 8
//     policies, not of all K. K < 8: policy k deals its tiles round-robin over the `spread` = 8 / K lanes
//     k spread .. k spread + spread - 1 (K = 1: the identity). A block whose position holds no tile returns.
// Placement is a matter of speed only: every tile is computed by exactly one block in either order.
struct MultiArgs {
  PolicyArgs a;
  int K, order, spread;
  int seg[DUCK_POLICY_MAX_POLICIES + 1];
  int start[DUCK_POLICY_MAX_POLICIES];
};

__global__ __launch_bounds__(256) void policy_act_kernel(MultiArgs m) {
  const int b = blockIdx.x;
  int k, tile;
  if (m.order == 0) {
    int lo = 0, hi = m.K - 1;  // the last k with start[k] <= b (an empty segment shares its start with the next)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (m.start[mid] <= b) lo = mid; else hi = mid - 1;
    }
    k = lo;
    tile = b - m.start[k];
  } else if (m.K >= 8) {
    const int pos = b >> 3;
    k = -1;
    tile = 0;
    for (int c = b & 7; c < m.K; c += 8) {
      const int t = pos - m.start[c];
      if (t >= 0 && t < (m.seg[c + 1] - m.seg[c] + TR - 1) / TR) {
        k = c;
        tile = t;
      }
    }
    if (k < 0) return;
  } else {
    const int lane = b & 7;
    k = lane / m.spread;
    if (k >= m.K) return;
    tile = (b >> 3) * m.spread + (lane - k * m.spread);
  }
  const int r0 = m.seg[k] + tile * TR, end = m.seg[k + 1];
  if (r0 >= end) return;
  policy_tile(m.a, r0, end, k);
}

int g_multi_order = 1;  // dealt over the XCDs: the faster one at K = 8 and K = 64 (DESIGN.md §9 "Policies")

// duck_policy_act's refusals and its launch arguments (what: the entry's name, for the message). 1: nothing to launch.
int policy_args(PolicyArgs& a, const char* what, int N, int nlayers, const int* sizes, const float* const* W,
                const float* const* b, const float* mean, const float* istd, const float* obs, float* logits,
                float* action) {
  char msg[128];
  auto fail = [&](const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return duck_fail(DUCK_EINVAL, msg);
  };
  if (N < 0 || nlayers < 1 || nlayers > DUCK_POLICY_MAX_LAYERS || !sizes) return fail("1 .. DUCK_POLICY_MAX_LAYERS layers");
  memset(&a, 0, sizeof(a));
  for (int l = 0; l <= nlayers; l++) {
    if (sizes[l] < 1 || sizes[l] > MAXW) return fail("every size in 1 .. 512");
    a.sizes[l] = sizes[l];
  }
  if (sizes[nlayers] & 1) return fail("the last size (loc | scale) must be even");
  if (N == 0) return 1;
  if (!W || !b || !obs || !action || (!mean) != (!istd)) return fail("null pointer");
  for (int l = 0; l < nlayers; l++) {
    if (!W[l] || !b[l]) return fail("null layer pointer");
    a.W[l] = W[l];
    a.b[l] = b[l];
    const int words = TR * ((sizes[l] + KC - 1) / KC * KC);  // layer l reads buffer l & 1
    if (words > a.buf_words[l & 1]) a.buf_words[l & 1] = words;
  }
  a.N = N;
  a.nl = nlayers;
  a.mean = mean;
  a.istd = istd;
  a.obs = obs;
  a.logits = logits;
  a.action = action;
  return DUCK_OK;
}

// The tables of `order` for the K segments of seg, then the launch (m.a filled by policy_args).
int policy_launch(MultiArgs& m, int K, const int* seg, int order, void* stream) {
  m.K = K;
  m.order = order;
  m.spread = K < 8 ? 8 / K : 1;
  for (int k = 0; k <= K; k++) m.seg[k] = seg[k];
  auto nt = [&](int k) { return (seg[k + 1] - seg[k] + TR - 1) / TR; };
  int blocks = 0;
  if (order == 0) {
    for (int k = 0; k < K; k++) {
      m.start[k] = blocks;
      blocks += nt(k);
    }
  } else if (K >= 8) {
    int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // positions taken in each lane
    for (int k = 0; k < K; k++) {
      m.start[k] = used[k & 7];
      used[k & 7] += nt(k);
    }
    for (int x = 0; x < 8; x++) blocks = used[x] * 8 > blocks ? used[x] * 8 : blocks;
  } else {
    for (int k = 0; k < K; k++) {
      const int pos = (nt(k) + m.spread - 1) / m.spread;
      blocks = pos * 8 > blocks ? pos * 8 : blocks;
    }
  }
  if (blocks == 0) return DUCK_OK;
  const size_t lds = sizeof(float) * (size_t)(2 * BS_WORDS + m.a.buf_words[0] + m.a.buf_words[1]);
  // up to 96 KB of LDS (two 512-wide buffers): above the 64 KB a launch may ask for without this
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_act_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(sizeof(float) * (2 * BS_WORDS + 2 * TR * MAXW)));
  HIPCHECK(attr);
  hipLaunchKernelGGL(policy_act_kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, m);
  HIPCHECK(hipGetLastError());
  return DUCK_OK;
}

}  // namespace

// one policy over rows [0, N): the K = 1 case, block b takes tile b
extern "C" int duck_policy_act(int N, int nlayers, const int* sizes, const float* const* W, const float* const* b,
                               const float* mean, const float* istd, const float* obs, float* logits, float* action,
                               void* stream) {
  MultiArgs m;
  memset(&m, 0, sizeof(m));
  const int rc = policy_args(m.a, "duck_policy_act", N, nlayers, sizes, W, b, mean, istd, obs, logits, action);
  if (rc) return rc < 0 ? rc : DUCK_OK;
  const int seg[2] = {0, N};
  return policy_launch(m, 1, seg, 0, stream);
}

extern "C" int duck_policy_multi_order(int order) {
  const int was = g_multi_order;
  if (order == 0 || order == 1) g_multi_order = order;
  return was;
}

extern "C" int duck_policy_act_multi(int N, int K, const int* seg, int nlayers, const int* sizes,
                                     const float* const* W, const float* const* b, const float* mean, const float* istd,
                                     const float* obs, float* logits, float* action, void* stream) {
  if (K < 1 || K > DUCK_POLICY_MAX_POLICIES)
    return duck_fail(DUCK_EINVAL, "duck_policy_act_multi: 1 .. DUCK_POLICY_MAX_POLICIES policies");
  if (N < 0 || !seg || seg[0] != 0 || seg[K] != N)
    return duck_fail(DUCK_EINVAL, "duck_policy_act_multi: seg[0] must be 0 and seg[K] must be N");
  for (int k = 0; k < K; k++)
    if (seg[k + 1] < seg[k]) return duck_fail(DUCK_EINVAL, "duck_policy_act_multi: seg must be non-decreasing");
  MultiArgs m;
  memset(&m, 0, sizeof(m));
  const int rc = policy_args(m.a, "duck_policy_act_multi", N, nlayers, sizes, W, b, mean, istd, obs, logits, action);
  if (rc) return rc < 0 ? rc : DUCK_OK;
  return policy_launch(m, K, seg, g_multi_order, stream);
}
