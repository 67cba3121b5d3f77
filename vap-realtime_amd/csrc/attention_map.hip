// attention_map_kernel: the attention weights themselves, P = softmax(Q.K^T / 16 + ALiBi, causal), which the reference returns with
// attention=True (MultiHeadAttention.forward, rvap/vap_main/modules.py:82-110) and which every attention kernel of the step keeps in
// registers.  Diagnostic path (vapx_transformer_maps): one launch next to an attention launch, reading that launch's own Q and K rows.
//
// One wave per (stream, channel, head, 32-query tile).  S = Q.K^T on the fp32 matrix cores with Q as operand A and K as operand B of
// v_mfma_f32_32x32x2_f32: the key index lands on the lane (col = lane & 31) and the 32 query rows in the 16 accumulator registers of the
// two lane halves (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), so one register of one half is 32 consecutive floats of a map row: every
// store instruction writes two 128-byte runs.  The k order of the contraction is free as long as both operands agree: lane half g holds
// columns 32 g .. 32 g + 31 of its row (eight 16-byte loads) and step t multiplies columns t and 32 + t.
//
// Exact softmax in two passes over the key tiles at or below the diagonal (<= 16 tiles of 32 keys, T <= 512): the first keeps a running
// (max, sum) per lane and register and merges the 32 lanes of a row once at the end, the second recomputes each score tile and stores
// exp(s - max) / sum.  Keys above the diagonal are stored as 0.0f, tiles wholly above it without any arithmetic.  Loads clamp their row
// to n - 1 (rows >= n of the buffers are never read), stores are predicated on row < n and key < n, destination offsets are 64-bit.
// The key fragment of the next tile is fetched under the current tile's MFMAs, and the blocks of an item are numbered from its last
// query tile down, so the waves with the most key tiles start first.  No LDS, no scratch.  The traffic is the map itself (4 n^2 bytes
// per head) against 2 x 32 MFMAs per computed tile.
#include <float.h>

#include "vap_kernels.h"

namespace {

// all-reduce (max) inside each 32-lane half: the DPP / swizzle steps of half_sum (common.h)
__device__ __forceinline__ float half_max(float v) {
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));    // quad_perm [1,0,3,2]
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));    // quad_perm [2,3,0,1]
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));   // row_half_mirror
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));   // row_mirror
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)));                    // lane ^ 16
  return v;
}

// K fragment of keys j0 .. j0 + 31 (row clamped to n - 1): columns 32 half .. 32 half + 31 of this lane's key
__device__ __forceinline__ void load_keys(f32x4 (&kf)[8], const float* kbase, int ldkv, int j0, int col, int n) {
  const int kj = min(j0 + col, n - 1);
  const float* kp = kbase + (long)kj * ldkv;
#pragma unroll
  for (int u = 0; u < 8; ++u) kf[u] = *(const f32x4*)(kp + 4 * u);
}

// one 32 x 32 tile of raw scores: the wave's 32 queries x the 32 keys of kf
__device__ __forceinline__ f32x16 score_tile(const f32x4 (&qf)[8], const f32x4 (&kf)[8]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[u][0], kf[u][0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[u][1], kf[u][1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[u][2], kf[u][2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[u][3], kf[u][3], acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace

__global__ __launch_bounds__(64) void attention_map_kernel(AttnMapArgs a) {
  const int n_qt = (a.T + 31) >> 5;
  const int item = blockIdx.x / n_qt, it = n_qt - 1 - (blockIdx.x - item * n_qt);   // item = (stream, channel, head); its long tiles start first
  const int h = item & 3, bc = item >> 2;
  const int n = a.bn[bc >> 1];
  const int i0 = it * 32;
  if (i0 >= n) return;
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const float slope = exp2f(-2.0f * (float)(h + 1));  // [1/4, 1/16, 1/64, 1/256]

  const int qi = min(i0 + col, n - 1);
  const float* qp = a.q + ((long)bc * a.T + qi) * a.ldq + h * 64 + half * 32;
  f32x4 qf[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) qf[u] = *(const f32x4*)(qp + 4 * u);
  const float* kbase = a.k + (long)(bc ^ a.swap_kv) * a.T * a.ldkv + h * 64 + half * 32;

  // pass 1: running (max, sum) of every row over this lane's keys; keys above the diagonal (only in tile `it`) take no part
  float mx[16], sm[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { mx[r] = -FLT_MAX; sm[r] = 0.f; }
  f32x4 kf[8], kn[8];                                      // this tile's keys and the next tile's, one tile ahead (tile 0 again for pass 2)
  load_keys(kf, kbase, a.ldkv, 0, col, n);
  for (int jt = 0; jt <= it; ++jt) {
    load_keys(kn, kbase, a.ldkv, jt < it ? (jt + 1) * 32 : 0, col, n);
    const f32x16 acc = score_tile(qf, kf);
#pragma unroll
    for (int u = 0; u < 8; ++u) kf[u] = kn[u];
    const int j = jt * 32 + col;
    const float bias = slope * (float)j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float v = fmaf(acc[r], 0.0625f, bias);
      const float e = __expf(-fabsf(v - mx[r]));            // first key of the lane: v - (-FLT_MAX) = +inf, e = 0, sum = 1
      const float s = v > mx[r] ? fmaf(sm[r], e, 1.0f) : sm[r] + e;
      if (j <= i) { sm[r] = s; mx[r] = fmaxf(mx[r], v); }
    }
  }
  // merge the 32 lanes of every row (key 0 is at or below every diagonal, so the row maximum is finite); sm becomes 1 / sum
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float m = half_max(mx[r]);
    const float s = half_sum(sm[r] * __expf(mx[r] - m));    // a lane without a key: exp(-FLT_MAX - m) = 0
    mx[r] = m;
    sm[r] = 1.0f / s;
  }

  // pass 2: recompute, normalise, store; then the zero tiles to the right of the diagonal tile
  float* dbase = a.dst + (long)bc * a.dst_slab + (long)h * a.dst_head;
  for (int jt = 0; jt <= it; ++jt) {
    if (jt < it) load_keys(kn, kbase, a.ldkv, (jt + 1) * 32, col, n);
    const f32x16 acc = score_tile(qf, kf);
#pragma unroll
    for (int u = 0; u < 8; ++u) kf[u] = kn[u];
    const int j = jt * 32 + col;
    const float bias = slope * (float)j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float v = fmaf(acc[r], 0.0625f, bias);
      const float p = j <= i ? __expf(v - mx[r]) * sm[r] : 0.0f;
      if (i < n && j < n) dbase[(long)i * a.dst_ld + j] = p;
    }
  }
  for (int jt = it + 1; jt * 32 < n; ++jt) {
    const int j = jt * 32 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (i < n && j < n) dbase[(long)i * a.dst_ld + j] = 0.0f;
    }
  }
}

hipError_t launch_attention_map(const AttnMapArgs& a, int B, hipStream_t st) {
  const int n_qt = (a.T + 31) / 32;
  if (n_qt > 16) return hipErrorInvalidValue;            // T <= 512 (vapx_create enforces it)
  hipLaunchKernelGGL(attention_map_kernel, dim3((unsigned)((long)B * 8 * n_qt)), dim3(64), 0, st, a);
  return hipGetLastError();
}
