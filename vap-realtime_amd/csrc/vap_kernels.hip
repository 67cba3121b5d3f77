// Non-GEMM kernels of the VAP step (gfx950): frame assembly + conv0, LSTM recurrence, context-ring
// gather + LayerNorm, causal ALiBi attention, combinator + heads.
#include "vap_kernels.h"

#include <cstdlib>

namespace {

// ------------------------------------------------------------------------------------------------
// 1. frame assembly + conv0 (1 -> 256, k10 s5 p3) + ChannelNorm + ReLU
//    reference: proc_serv_in carry logic vap_main.py:397-409; CPCEncoder.conv0/batchNorm0
//    encoder_components.py:83-84,99; ChannelNorm 64-70 (unbiased variance).
//    K = 10 is too thin for MFMA: one wave computes one output position (256 channels, 4 per lane)
//    with the 40 taps*channels weights held in registers; the channel reduction is a wave butterfly.
// ------------------------------------------------------------------------------------------------
// the P0 output positions of one assembled frame xs[L] -> outb[P0][256] (one wave per position)
__device__ __forceinline__ void conv0_positions(const float* xs, int L, const float* __restrict__ cw, const float* __restrict__ cbias,
                                                const float* __restrict__ cgamma, const float* __restrict__ cbeta, float* outb, int lane, int wave) {
  const int ch = lane * 4;
  f32x4 w[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) w[t] = *(const f32x4*)(cw + t * 256 + ch);
  const f32x4 bias = *(const f32x4*)(cbias + ch);
  const f32x4 gam = *(const f32x4*)(cgamma + ch);
  const f32x4 bet = *(const f32x4*)(cbeta + ch);
  const int P0 = L / 5;
  for (int p = wave; p < P0; p += 4) {
    f32x4 v = bias;
    const int x0 = p * 5 - 3;
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      int xi = x0 + t;
      float xv = (xi >= 0 && xi < L) ? xs[xi] : 0.f;
      v += w[t] * xv;
    }
    float s = wave_sum(v[0] + v[1] + v[2] + v[3]);
    float mean = s * (1.0f / 256.0f);
    f32x4 d = v - mean;
    float ss = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
    float rstd = rsqrtf(ss * (1.0f / 255.0f) + 1e-5f);
    f32x4 y = d * rstd * gam + bet;
    y[0] = relu_nanprop(y[0]); y[1] = relu_nanprop(y[1]); y[2] = relu_nanprop(y[2]); y[3] = relu_nanprop(y[3]);
    *(f32x4*)(outb + (long)p * 256 + ch) = y;
  }
}

__global__ __launch_bounds__(256) void conv0_kernel(Conv0Args a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [L]
  const int bc = blockIdx.x, b = bc >> 1, c = bc & 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sid = a.ids ? a.ids[b] : b;
  const int L = a.L, hop = L - VAPX_PAD;
  float* cr = a.carry ? a.carry + ((long)sid * 2 + c) * VAPX_PAD : nullptr;
  if (a.spc == hop) {
    for (int i = tid; i < VAPX_PAD; i += 256) xs[i] = cr[i];
    const float* src = a.audio + ((long)b * 2 + c) * hop;
    for (int i = tid; i < hop; i += 256) xs[VAPX_PAD + i] = src[i];
  } else {
    const float* src = a.audio + ((long)b * 2 + c) * L;
    for (int i = tid; i < L; i += 256) xs[i] = src[i];
  }
  __syncthreads();
  if (cr)
    for (int i = tid; i < VAPX_PAD; i += 256) cr[i] = xs[L - VAPX_PAD + i];
  if (a.frames_seen && c == 0 && tid == 0) {
    int fs = a.frames_seen[sid];
    a.bn[b] = fs + 1 < a.T ? fs + 1 : a.T;
    a.bhead[b] = fs % a.T;
  }

  conv0_positions(xs, L, a.w, a.bias, a.gamma, a.beta, a.h0 + (long)bc * (L / 5 + 4) * 256 + 2 * 256, lane, wave);
}

// vapx_prefill: the same conv0 over (frame, stream) pairs cut from a contiguous block.  Frame j of a row starts hop * j samples in and is
// prefixed by the 320 samples in front of it - the block's own, or for the call's very first frame the stream's carry.  Nothing is written
// but h0 and, by a call's first chunk, the ring slot of the call's first frame (bhead, as the step's conv0 publishes it): the carry and the
// frame counter move once, in the ring fill of the call's last chunk - no launch both reads and writes either.
__global__ __launch_bounds__(256) void conv0_kernel(Conv0PrefillArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [L]
  const int vc = blockIdx.x, v = vc >> 1, c = vc & 1, j = v / a.n, k = v - j * a.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = a.L, hop = L - VAPX_PAD;
  const float* row = a.audio + ((long)k * 2 + c) * a.row_stride + (long)j * hop;
  const float* pre = row - VAPX_PAD;
  if (j == 0 && !a.prefix_in_audio) pre = a.carry + ((long)(a.ids ? a.ids[k] : k) * 2 + c) * VAPX_PAD;
  for (int i = tid; i < VAPX_PAD / 4; i += 256) ((f32x4*)xs)[i] = ((const f32x4*)pre)[i];
  for (int i = tid; i < hop / 4; i += 256) ((f32x4*)(xs + VAPX_PAD))[i] = ((const f32x4*)row)[i];
  if (a.bhead && j == 0 && c == 0 && tid == 0) a.bhead[k] = a.frames_seen[a.ids ? a.ids[k] : k] % a.T;
  __syncthreads();
  conv0_positions(xs, L, a.w, a.bias, a.gamma, a.beta, a.h0 + (long)vc * (L / 5 + 4) * 256 + 2 * 256, lane, wave);
}

// ------------------------------------------------------------------------------------------------
// 2. LSTM (256 -> 256, 1 layer), n_cpc sequential steps, persistent (h, c), + fused downsample
//    reference: CPCAR.forward encoder_components.py:140-159 (nn.LSTM, gate order i,f,g,o, both
//    biases), keepHidden=True (encoder.py:27); downsample get_cnn_layer :496-511 with the weight
//    swapped in at vap_main.py:204-212: Conv1d(256,256,K=n_cpc) over exactly n_cpc frames = one
//    dense [n_cpc*256 -> 256] contraction, then LayerNorm + exact GELU.
//    The input projection z.W_ih^T + b_ih + b_hh for all steps is a plain batched GEMM (engine:
//    gx); only h_{t-1}.W_hh^T (K = 256) is sequential.  One workgroup = 16 (stream,channel) rows
//    (v_mfma_f32_16x16x4_f32 so that a small batch still spreads over CUs), 8 waves; wave w owns
//    hidden units 32w..32w+31 for all four gates (weight rows pre-permuted: its 128 columns are
//    [i|f|g|o] x 32 -> the cell update is lane-local).  h lives in LDS between steps, c in registers,
//    W_hh / W_down fragments stream from L2 in fragment-major order.  The downsample contribution of
//    step t (h_t . Wd_t^T) rides in the MFMA phase of step t+1, which reads the same h_t from LDS.
// ------------------------------------------------------------------------------------------------
constexpr int H_LD = 260;  // 256 + 4 pad floats
typedef float f32x4v __attribute__((ext_vector_type(4)));

// One source for the step (kPrefill = false: lstm_kernel, the code it always was) and for vapx_prefill (kPrefill = true): the same cell
// step walks a.frames frames in one launch - h stays in LDS and c in registers across the frame boundaries, both register rings wrap
// into the next frame as they wrap between steps, and the downsample + LN + GELU (+ LN0) epilogue runs once per frame on that frame's
// block of e / en.  State is written once, after the last frame.  The arguments travel by value and the frame loop is a do-while
// whose condition the step folds away: with a reference or a counted loop the step's instantiation came out with other SGPR and
// instruction counts than the kernel it replaces (now 216 VGPRs, 56 SGPRs, 2 104 instructions, as before; profiles/prefill/README.md).
template <bool kPrefill, typename Args>
__device__ __forceinline__ void lstm_body(const Args a) {
  __shared__ __attribute__((aligned(16))) float hbuf[16 * H_LD];
  __shared__ float red[8 * 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar wave index -> SGPR-based fragment addressing
  const int l15 = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * 16;

  auto state_row = [&](int m) {
    m = m < a.M ? m : a.M - 1;
    int b = m >> 1;
    int sid = a.ids ? a.ids[b] : b;
    return (long)sid * 2 + (m & 1);
  };
  for (int i = tid; i < 16 * 64; i += 512) {
    int row = i >> 6, q = (i & 63) * 4;
    *(f32x4*)&hbuf[row * H_LD + q] = *(const f32x4*)(a.h_state + state_row(m0 + row) * 256 + q);
  }
  // accumulator (ns, reg): row = 4*kq + reg, column ns*16 + l15 of this wave's 128 = gate ns/2,
  // hidden unit j = 32w + 16*(ns&1) + l15.  c for (q = ns&1, reg) stays in registers.
  float creg[2][4];
  long srow[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    srow[reg] = state_row(m0 + kq * 4 + reg);
#pragma unroll
    for (int q = 0; q < 2; ++q) creg[q][reg] = a.c_state[srow[reg] * 256 + w * 32 + q * 16 + l15];
  }
  const f32x4* wf = (const f32x4*)a.wfrag + (long)w * 16 * 8 * 64;      // [8 w][16 kc][8 ns][64], wave-uniform
  const f32x4* df = (const f32x4*)a.down_wf + (long)w * 16 * 2 * 64;     // [T][8 w][16 kc][2 ns][64]
  const float* pa = &hbuf[l15 * H_LD + kq * 4];
  // W_hh fragments run through a register ring 2 kc (= 64 MFMAs) ahead of their use; since every
  // step multiplies by the same W_hh the ring simply wraps from kc 15 to kc 0 of the next step, so
  // the L2 latency is never exposed — not even at step boundaries.
  f32x4 ring[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) ring[i] = wf[i * 64 + lane];
  f32x4 dring[4];
  if (a.down_wf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dring[i] = df[i * 64 + lane];
  }
  f32x4v dacc[2] = {f32x4v{0.f, 0.f, 0.f, 0.f}, f32x4v{0.f, 0.f, 0.f, 0.f}};
  auto down_step = [&](int t) {   // dacc += h_t (in hbuf) . Wd_t^T for this wave's 32 output columns
    const f32x4* d = df + (long)t * 8 * 16 * 2 * 64;
    const f32x4* dn = df + (long)(t + 1 < a.ncpc ? t + 1 : (kPrefill ? 0 : t)) * 8 * 16 * 2 * 64;   // prefill: on into the next frame's step 0
#pragma unroll 1
    for (int kp = 0; kp < 8; ++kp) {
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int kc = kp * 2 + h2;
        f32x4 av = *(const f32x4*)(pa + kc * 16);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          dacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], dring[h2 * 2][s], dacc[0], 0, 0, 0);
          dacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], dring[h2 * 2 + 1][s], dacc[1], 0, 0, 0);
        }
        const f32x4* nx = kc + 2 < 16 ? d + ((kc + 2) * 2) * 64 : dn + ((kc + 2 - 16) * 2) * 64;
        dring[h2 * 2] = nx[lane];
        dring[h2 * 2 + 1] = nx[64 + lane];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  int n_frames = 1;
  if constexpr (kPrefill) n_frames = a.frames;
  const float* gxf = a.gx;   // this frame's blocks of gx / e / en
  float *ef = a.e, *enf = a.en;
  int f = 0;
  do {   // frames: one pass in the step, whose loop condition is a constant false
  if constexpr (kPrefill) dacc[0] = dacc[1] = f32x4v{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < a.ncpc; ++t) {
    // this step's input projection (issued early: in flight under the MFMAs)
    float gxr[4][8];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int m = m0 + kq * 4 + reg;
      m = m < a.M ? m : a.M - 1;
      const float* gx = gxf + ((long)m * a.ncpc + t) * 1024 + w * 128 + l15;
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8) gxr[reg][c8] = gx[c8 * 16];
    }
    __syncthreads();  // hbuf holds h_{t-1}
    f32x4v acc[8];
#pragma unroll
    for (int ns = 0; ns < 8; ++ns) acc[ns] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kp = 0; kp < 8; ++kp) {
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int kc = kp * 2 + h2;
        f32x4 av = *(const f32x4*)(pa + kc * 16);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int ns = 0; ns < 8; ++ns)
            acc[ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], ring[h2 * 8 + ns][s], acc[ns], 0, 0, 0);
        const f32x4* nx = wf + (long)(((kc + 2) & 15) * 8) * 64;
#pragma unroll
        for (int ns = 0; ns < 8; ++ns) ring[h2 * 8 + ns] = nx[ns * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);   // keep the refill behind its MFMAs (hipcc would sink it)
      }
    }
    if (t > 0 && a.down_wf) down_step(t - 1);
    __syncthreads();  // every wave has finished reading hbuf for this step
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = kq * 4 + reg;
      const int m = m0 + row;
      const bool live = m < a.M;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float ig = fast_sigmoid(acc[0 + q][reg] + gxr[reg][0 + q]);
        float fg = fast_sigmoid(acc[2 + q][reg] + gxr[reg][2 + q]);
        float gg = fast_tanh(acc[4 + q][reg] + gxr[reg][4 + q]);
        float og = fast_sigmoid(acc[6 + q][reg] + gxr[reg][6 + q]);
        float cn = fg * creg[q][reg] + ig * gg;
        creg[q][reg] = cn;
        float hn = og * fast_tanh(cn);
        const int j = w * 32 + q * 16 + l15;
        hbuf[row * H_LD + j] = hn;
        if (!kPrefill && live) a.out[((long)m * a.ncpc + t) * 256 + j] = hn;
      }
    }
  }
  __syncthreads();
  if (!kPrefill || f + 1 == n_frames) {
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = kq * 4 + reg;
    if (m0 + row < a.M) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = w * 32 + q * 16 + l15;
        a.c_state[srow[reg] * 256 + j] = creg[q][reg];
        a.h_state[srow[reg] * 256 + j] = hbuf[row * H_LD + j];
      }
    }
  }
  }
  if (!a.down_wf) return;
  // ---- downsample epilogue: + bias, LayerNorm over 256 outputs (8 waves), exact GELU -> e ----
  down_step(a.ncpc - 1);
  const int oc = w * 32 + l15;                       // output columns oc, oc + 16
  const float b0 = a.down_b[oc], b1 = a.down_b[oc + 16];
  float s[4], mean[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    dacc[0][reg] += b0;
    dacc[1][reg] += b1;
    float t = dacc[0][reg] + dacc[1][reg];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o);   // 16 lanes that share kq
    s[reg] = t;
  }
  if (l15 == 0)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[w * 16 + kq * 4 + reg] = s[reg];
  __syncthreads();
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) t += red[u * 16 + kq * 4 + reg];
    mean[reg] = t * (1.0f / 256.0f);
  }
  __syncthreads();
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float d0 = dacc[0][reg] - mean[reg], d1 = dacc[1][reg] - mean[reg];
    float t = d0 * d0 + d1 * d1;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o);
    s[reg] = t;
  }
  if (l15 == 0)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[w * 16 + kq * 4 + reg] = s[reg];
  __syncthreads();
  const float g0 = a.down_g[oc], g1 = a.down_g[oc + 16], be0 = a.down_beta[oc], be1 = a.down_beta[oc + 16];
  float ev[2][4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) t += red[u * 16 + kq * 4 + reg];
    const float rstd = rsqrtf(t * (1.0f / 256.0f) + 1e-5f);
    const int m = m0 + kq * 4 + reg;
    ev[0][reg] = gelu_erf((dacc[0][reg] - mean[reg]) * rstd * g0 + be0);
    ev[1][reg] = gelu_erf((dacc[1][reg] - mean[reg]) * rstd * g1 + be1);
    if (m < a.M) {
      ef[(long)m * 256 + oc] = ev[0][reg];
      ef[(long)m * 256 + oc + 16] = ev[1][reg];
    }
  }
  if (!a.en) return;
  // ---- en = LayerNorm(e; ln_self of transformer layer 0): input of the cached layer-0 Q/K/V ----
  auto rows_allsum = [&](float(&v)[4]) {   // sum over the 256 columns of each of this lane's 4 rows
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float t = v[reg];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o);
      v[reg] = t;
    }
    __syncthreads();
    if (l15 == 0)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) red[w * 16 + kq * 4 + reg] = v[reg];
    __syncthreads();
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      float t = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) t += red[u * 16 + kq * 4 + reg];
      v[reg] = t;
    }
  };
  float sm[4], sv[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) sm[reg] = ev[0][reg] + ev[1][reg];
  rows_allsum(sm);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    sm[reg] *= (1.0f / 256.0f);
    float d0 = ev[0][reg] - sm[reg], d1 = ev[1][reg] - sm[reg];
    sv[reg] = d0 * d0 + d1 * d1;
  }
  rows_allsum(sv);
  const float lg0 = a.ln0_g[oc], lg1 = a.ln0_g[oc + 16], lb0 = a.ln0_b[oc], lb1 = a.ln0_b[oc + 16];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float rstd = rsqrtf(sv[reg] * (1.0f / 256.0f) + 1e-5f);
    const int m = m0 + kq * 4 + reg;
    if (m < a.M) {
      enf[(long)m * 256 + oc] = (ev[0][reg] - sm[reg]) * rstd * lg0 + lb0;
      enf[(long)m * 256 + oc + 16] = (ev[1][reg] - sm[reg]) * rstd * lg1 + lb1;
    }
  }
  if constexpr (kPrefill) {
    gxf += (long)a.M * a.ncpc * 1024;
    ef += (long)a.M * 256;
    enf += (long)a.M * 256;
  }
  } while (kPrefill && ++f < n_frames);
}

__global__ __launch_bounds__(512) void lstm_kernel(LstmArgs a) { lstm_body<false>(a); }
__global__ __launch_bounds__(512) void lstm_kernel(LstmPrefillArgs a) { lstm_body<true>(a); }

// ------------------------------------------------------------------------------------------------
// 3. context-ring append + chronological gather + LayerNorm(ln_self of layer 0)
//    reference: vap_main.py:274-283 (append, keep last T, cat).  One wave per row.
// ------------------------------------------------------------------------------------------------
// ring-direct mode: append this frame's embedding and layer-0 Q|K|V to the rings and publish the
// rotation that maps logical (chronological) rows to ring slots; nothing else moves.  One wave per
// (stream, channel).
__global__ __launch_bounds__(256) void ring_append_kernel(GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int bc = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bc >= a.B * 2) return;
  const int b = bc >> 1, c = bc & 1;
  const int sid = a.ids ? a.ids[b] : b;
  const int head = a.bhead[b], n = a.bn[b];
  float* rb = a.ring + ((long)sid * 2 + c) * a.T * 256;
  float* rq = a.ring_qkv + ((long)sid * 2 + c) * a.T * 768;
  *(f32x4*)(rb + (long)head * 256 + lane * 4) = *(const f32x4*)(a.e + (long)bc * 256 + lane * 4);
  const float* qn = a.qkv_new + (long)bc * 768 + lane * 4;
  float* qs = rq + (long)head * 768 + lane * 4;
  *(f32x4*)(qs) = *(const f32x4*)(qn);
  *(f32x4*)(qs + 256) = *(const f32x4*)(qn + 256);
  *(f32x4*)(qs + 512) = *(const f32x4*)(qn + 512);
  if (c == 0 && lane == 0) {
    int rot = head + 1 - n;           // slot of the oldest row
    a.rot[b] = rot < 0 ? rot + a.T : rot;
  }
}

// vapx_prefill: a chunk's embeddings and layer-0 Q|K|V rows into their ring slots, one wave per (frame, stream, channel) row, 16 bytes per
// lane and access.  Frame g of the call goes to slot (bhead + g) % T, bhead being the slot of the call's first frame (conv0 of the first
// chunk).  Within a call the slots of the written frames are distinct (a frame that a later one overwrites is skipped, here or as a
// whole chunk on the host), so no two waves of a launch meet.  The waves of the call's last frame also move the carry (the block's last
// 320 samples) and the frame counter, which no other wave of this launch reads.
__global__ __launch_bounds__(256) void ring_append_kernel(PrefillFillArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.fc * a.n * 2) return;
  const int c = r & 1, v = r >> 1;
  const int j = v / a.n, k = v - j * a.n;
  const int g = a.f0 + j;
  if ((long)g + a.T < a.frames) return;
  const int sid = a.ids ? a.ids[k] : k;
  const int slot = (int)(((long)a.bhead[k] + g) % a.T);
  float* rb = a.ring + (((long)sid * 2 + c) * a.T + slot) * 256 + lane * 4;
  float* qs = a.ring_qkv + (((long)sid * 2 + c) * a.T + slot) * 768 + lane * 4;
  *(f32x4*)rb = *(const f32x4*)(a.e + (long)r * 256 + lane * 4);
  const float* qn = a.qkv_new + (long)r * 768 + lane * 4;
  *(f32x4*)(qs) = *(const f32x4*)(qn);
  *(f32x4*)(qs + 256) = *(const f32x4*)(qn + 256);
  *(f32x4*)(qs + 512) = *(const f32x4*)(qn + 512);
  if (g + 1 != a.frames) return;
  const f32x4* src = (const f32x4*)(a.tail + ((long)k * 2 + c) * a.row_stride);
  f32x4* dst = (f32x4*)(a.carry + ((long)sid * 2 + c) * VAPX_PAD);
  dst[lane] = src[lane];
  if (lane < VAPX_PAD / 4 - 64) dst[64 + lane] = src[64 + lane];
  if (c == 0 && lane == 0) a.frames_seen[sid] += a.frames;
}

__global__ __launch_bounds__(256) void gather_ln_kernel(GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)a.B * 2 * a.T) return;
  const int t = (int)(row % a.T);
  const int bc = (int)(row / a.T), b = bc >> 1, c = bc & 1;
  const int n = a.bn[b];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  f32x4 q0 = v, q1 = v, q2 = v;
  if (t < n) {
    if (a.ring) {
      const int sid = a.ids ? a.ids[b] : b;
      const int head = a.bhead[b];
      float* rb = a.ring + ((long)sid * 2 + c) * a.T * 256;
      float* rq = a.ring_qkv ? a.ring_qkv + ((long)sid * 2 + c) * a.T * 768 : nullptr;
      if (t == n - 1) {
        v = *(const f32x4*)(a.e + (long)bc * 256 + lane * 4);
        *(f32x4*)(rb + (long)head * 256 + lane * 4) = v;
        if (rq) {
          const float* qn = a.qkv_new + (long)bc * 768 + lane * 4;
          q0 = *(const f32x4*)(qn); q1 = *(const f32x4*)(qn + 256); q2 = *(const f32x4*)(qn + 512);
          float* qs = rq + (long)head * 768 + lane * 4;
          *(f32x4*)(qs) = q0; *(f32x4*)(qs + 256) = q1; *(f32x4*)(qs + 512) = q2;
        }
      } else {
        int slot = head + 1 - n + t;
        slot = slot < 0 ? slot + a.T : slot;
        v = *(const f32x4*)(rb + (long)slot * 256 + lane * 4);
        if (rq) {
          const float* qs = rq + (long)slot * 768 + lane * 4;
          q0 = *(const f32x4*)(qs); q1 = *(const f32x4*)(qs + 256); q2 = *(const f32x4*)(qs + 512);
        }
      }
    } else {
      v = *(const f32x4*)(a.xin + ((long)bc * a.rows_in + t) * 256 + lane * 4);
    }
  }
  *(f32x4*)(a.x0 + row * 256 + lane * 4) = v;
  if (a.ring && a.ring_qkv) {   // layer-0 Q/K/V come from the per-row cache: no LayerNorm / GEMM needed
    float* qo = a.qkv + row * 768 + lane * 4;
    *(f32x4*)(qo) = q0; *(f32x4*)(qo + 256) = q1; *(f32x4*)(qo + 512) = q2;
    return;
  }
  float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
  f32x4 d = v - mean;
  float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 256.0f);
  float rstd = rsqrtf(var + 1e-5f);
  f32x4 g = *(const f32x4*)(a.gamma + lane * 4), be = *(const f32x4*)(a.beta + lane * 4);
  *(f32x4*)(a.xn + row * 256 + lane * 4) = d * rstd * g + be;
}

// ------------------------------------------------------------------------------------------------
// 4. causal multi-head attention with ALiBi key bias, fp32 MFMA
//    reference: MultiHeadAttention.forward modules.py:82-110 (scale 1/sqrt(dim)=1/16, :52),
//    MultiHeadAttentionAlibi.get_alibi_mask 162-188 (bias m_h * j on the KEY index).
//    One workgroup per (stream, channel, head); K and V tiles [n][64] staged in LDS (zero rows
//    beyond n).  Each wave owns 32-query tiles `it` and computes the TRANSPOSED score tile
//        S^T[j][i] = sum_d K[j][d] Q[i][d]          (A = K from LDS, B = Q from global)
//    for the causal key tiles jt <= it.  In the 32x32 accumulator layout a query column i then
//    lives in ONE lane pair (l, l+32): the softmax row max / sum are lane-local plus one
//    cross-half shuffle, and — the point of transposing — accumulator register r of S^T is
//    exactly the B operand of MFMA step r of   O^T[d][i] = sum_j V[j][d] P^T[j][i]
//    (lane half h holds key j0(r)+4h, which is the k-slot that half supplies), so P never moves.
// ------------------------------------------------------------------------------------------------
// Long windows (64 < T <= 256): TWO workgroups per CU so that one workgroup's V staging / Q loads / output stores hide behind the
// other's MFMAs.  Only V sits in LDS (64 KB for 256 keys, unpadded: its reads are lane-consecutive); K fragments come straight from
// global / L2 as the MFMA A operand (as in attn_block_kernel), double-buffered one key tile ahead; the softmax is online per 32-key
// tile, so one score accumulator is live (~190 registers).  Four waves, each takes query tiles w and 7 - w (9 causal key tiles per
// wave: balanced).  Optional ring addressing lets layer 0 read the per-stream Q|K|V rings in place (no chronological gather).
// (Two earlier generations — K+V in LDS with 4 and with 8 waves — are in the history: profiles/r02_experiments/c3_attention_*.json.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attention_long2_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Vs[];   // [n_tiles * 32][64]
  const int T = a.T;
  const int n_tiles = (T + 31) >> 5;                 // <= 8
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = (int)(blockIdx.x & 3), bc = (int)(blockIdx.x >> 2), b = bc >> 1;
  const int n = a.bn[b];
  const int kvbc = a.swap_kv ? (bc ^ 1) : bc;
  const int l31 = lane & 31, hi = lane >> 5;
  const bool ringed = a.ring_rot != nullptr;
  const int rot = ringed ? a.ring_rot[b] : 0;
  const long slab_q = ringed ? ((long)(a.ids ? a.ids[b] : b) * 2 + (bc & 1)) : (long)bc;
  const long slab_kv = ringed ? slab_q : (long)kvbc;
  auto prow = [&](int i) { int r = i + rot; return r >= T ? r - T : r; };
  const float* kp = a.k + slab_kv * T * a.ldkv + h * 64;
  const float* vp = a.v + slab_kv * T * a.ldkv + h * 64;
  const int nt_valid = (n + 31) >> 5;
#ifdef VAPX_TRACE
  int stamp_k = 0;
  auto STAMP = [&]() {   // phase time stamps of wave 0 (debug build `make trace`: tools/attn_trace.py --long)
    if (a.trace && tid == 0 && stamp_k < 28 && blockIdx.x < 16384) a.trace[(long)blockIdx.x * 32 + stamp_k] = __builtin_amdgcn_s_memtime();
    ++stamp_k;
  };
  STAMP();   // 0: entry
  if (a.trace && tid == 0 && blockIdx.x < 16384) a.trace[(long)blockIdx.x * 32 + 28] = __builtin_amdgcn_s_memrealtime();
  // fine stamps of the start-up (round 6): the stamp is taken once `x` has ARRIVED (an empty asm that consumes it pins the s_waitcnt there)
#define STAMP_WHEN(x) do { asm volatile("" ::"v"(x)); STAMP(); } while (0)
  STAMP_WHEN(n + rot);   // 1: per-stream metadata (window fill, ring rotation) loaded
#else
  auto STAMP = [] {};
#define STAMP_WHEN(x) do { } while (0)
#endif
  // The V tile (up to 256 keys x 64 features of this head) goes to LDS, but NOTHING waits for it before the first score tile is done:
  // all 16 loads of a lane are issued first, then this wave's Q and K fragments, then S = K.Q^T of key tile 0 and its softmax run while
  // V is still in flight; only then V lands in LDS (one barrier) and the P.V products start.  (Round 2 staged V in a load -> store loop
  // ahead of everything else: 5.6 us alone, 18 us of a 47 us workgroup under load — profiles/r03_experiments/attn_long_trace_*.)
  f32x4 vv[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int idx = u * 256 + tid, j = idx >> 4, q = (idx & 15) * 4;
    const int jc = j < n ? j : n - 1;
    vv[u] = *(const f32x4*)(vp + (long)prow(jc) * a.ldkv + q);
  }
  const float slope = exp2f(-2.0f * (float)(h + 1));  // [1/4, 1/16, 1/64, 1/256]
  const float hi4f = (float)(4 * hi);
  auto load_k = [&](f32x4 (&kf)[8], int jt) {          // A operand of S^T = K.Q^T: key row jt*32 + l31, k-slots kc*8 + 4*hi ..+3
    int j = jt * 32 + l31;
    j = j < n ? j : n - 1;                             // rows beyond the window: clamped, masked below
    const float* kr = kp + (long)prow(j) * a.ldkv + hi * 4;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) kf[kc] = *(const f32x4*)(kr + kc * 8);
  };
  auto load_q = [&](f32x4 (&qf)[8], int it) {          // B operand: query row it*32 + l31 (clamped), k-slots kc*8 + 4*hi ..+3
    int i = it * 32 + l31;
    i = i < n ? i : n - 1;
    const float* qp = a.q + (slab_q * T + prow(i)) * a.ldq + h * 64 + hi * 4;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) qf[kc] = *(const f32x4*)(qp + kc * 8);
  };
  f32x4 qf[8], qn[8], kfa[8], kfb[8];
  float m = -1e30f, l = 0.f;
  f32x16 o0, o1, sc;
  auto scores = [&](const f32x4 (&kf)[8]) {   // S^T tile = K_tile . Q^T: 32 MFMAs into one accumulator (unscaled: the 1/16 rides in the softmax fma)
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc)
#pragma unroll
      for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[kc][s], qf[kc][s], sc, 0, 0, 0);
  };
  // online softmax update for one 32-key tile: sc := P, returns the rescale factor of the running output.  accumulator r <-> key
  // j = 32 jt + C_r + 4 hi with C_r = (r&3) + 8 (r>>2) a constant.  MASKED only for the tiles that need it: the diagonal tile
  // (causal) and the tile that holds the window end; interior tiles skip the compares and selects.
  auto softmax = [&](int jt, int i, bool masked) {
    float cm = -1e30f;
    const float jb = (float)(jt * 32) + hi4f;
    if (masked) {
      const int i4 = i - jt * 32 - 4 * hi, n4 = n - jt * 32 - 4 * hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2);
        float v = fmaf(sc[r], 0.0625f, slope * ((float)c + jb));
        v = ((c <= i4) && (c < n4)) ? v : -1e30f;
        sc[r] = v;
        cm = fmaxf(cm, v);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2);
        const float v = fmaf(sc[r], 0.0625f, slope * ((float)c + jb));
        sc[r] = v;
        cm = fmaxf(cm, v);
      }
    }
    cm = fmaxf(cm, __shfl_xor(cm, 32));
    const float mn = fmaxf(m, cm);
    const float alpha = __expf(m - mn);
    float sum = 0.f;
    if (masked) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = sc[r] > -1e29f ? __expf(sc[r] - mn) : 0.f;
        sc[r] = pv;
        sum += pv;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __expf(sc[r] - mn);
        sc[r] = pv;
        sum += pv;
      }
    }
    sum += __shfl_xor(sum, 32);
    l = l * alpha + sum;
    m = mn;
    return alpha;
  };
  auto pv = [&](int jt, float alpha) {  // O^T = alpha O^T + V_tile^T . P^T
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* va = &Vs[(jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * 64 + l31];
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[0], sc[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[32], sc[r], o1, 0, 0, 0);
    }
  };
  auto needs_mask = [&](int jt, int it) { return jt == it || (jt + 1) * 32 > n; };
  auto begin = [&]() {
    m = -1e30f; l = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  };
  // key tiles jt0 .. it of query tile `it`; kfa / kfb already hold tiles jt0 / jt0 + 1 (fragments ping-pong one tile ahead of their use)
  auto tiles_from = [&](int jt0, int it) {
#pragma unroll 1
    for (int jt = jt0; jt <= it; jt += 2) {
      scores(kfa);
      if (jt + 2 <= it) load_k(kfa, jt + 2);
      float al = softmax(jt, it * 32 + l31, needs_mask(jt, it));
      pv(jt, al);
      if (jt + 1 <= it) {
        scores(kfb);
        if (jt + 3 <= it) load_k(kfb, jt + 3);
        al = softmax(jt + 1, it * 32 + l31, needs_mask(jt + 1, it));
        pv(jt + 1, al);
      }
    }
  };
  auto store_tile = [&](int it) {
    const int i = it * 32 + l31;
    float* op = a.out + ((long)bc * T + i) * 256 + h * 64;
    if (i < T) {
      const float scl = i < n ? 1.0f / l : 0.f;         // rows beyond the valid window: deterministic zeros
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        f32x4 v0 = {o0[rr * 4 + 0], o0[rr * 4 + 1], o0[rr * 4 + 2], o0[rr * 4 + 3]};
        f32x4 v1 = {o1[rr * 4 + 0], o1[rr * 4 + 1], o1[rr * 4 + 2], o1[rr * 4 + 3]};
        *(f32x4*)(op + rr * 8 + hi * 4) = v0 * scl;
        *(f32x4*)(op + 32 + rr * 8 + hi * 4) = v1 * scl;
      }
    }
  };
  auto zero_tile = [&](int it) {                          // whole tile beyond the valid rows: deterministic zeros
    const int i = it * 32 + l31;
    if (i < T) {
      float* op = a.out + ((long)bc * T + i) * 256 + h * 64;
#pragma unroll
      for (int d = 0; d < 8; ++d) *(f32x4*)(op + hi * 32 + d * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  // ---- pass 0 prologue: query tile w against key tile 0, before V is needed ----
  const int it0 = w, it1 = 7 - w;
  const bool act0 = it0 < nt_valid, act1 = it1 < nt_valid;
  float al0 = 0.f;
  if (act0) {
    load_q(qf, it0);
    load_k(kfa, 0);
    if (it0 >= 1) load_k(kfb, 1);
    begin();
    STAMP_WHEN(qf[7][3] + kfa[7][3]);   // 2: this wave's Q fragments and K tile 0 arrived (in-order returns: the 16 V loads issued before them too)
    scores(kfa);
    if (it0 >= 2) load_k(kfa, 2);
    al0 = softmax(0, it0 * 32 + l31, needs_mask(0, it0));
    STAMP_WHEN(al0);                    // 3: first score tile + softmax done
  }
  if (act1) load_q(qn, it1);                             // the second pass's Q fragments fly under the first pass
  // ---- V tile -> LDS (rows >= n: zeros; masked keys have P = 0 exactly, and 0 x garbage must stay 0) ----
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int idx = u * 256 + tid, j = idx >> 4, q = (idx & 15) * 4;
    if (j < nt_valid * 32) *(f32x4*)&Vs[j * 64 + q] = j < n ? vv[u] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  STAMP();   // 4: this wave's part of V written to LDS
  __syncthreads();
  STAMP();   // 5: barrier passed (every wave's first score tile done, whole V tile staged)
  if (act0) {
    pv(0, al0);
    if (it0 >= 1) {   // kfb holds tile 1, kfa tile 2: continue with (kfb, kfa) swapped roles
      scores(kfb);
      if (it0 >= 3) load_k(kfb, 3);
      float al = softmax(1, it0 * 32 + l31, needs_mask(1, it0));
      pv(1, al);
      tiles_from(2, it0);
    }
    store_tile(it0);
  } else if (it0 < n_tiles) {
    zero_tile(it0);
  }
  STAMP();   // 6: query tile w done
  // ---- pass 1: query tile 7 - w ----
  if (act1) {
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) qf[kc] = qn[kc];
    load_k(kfa, 0);
    if (it1 >= 1) load_k(kfb, 1);
    begin();
    tiles_from(0, it1);
    store_tile(it1);
  } else if (it1 < n_tiles) {
    zero_tile(it1);
  }
  STAMP();   // 7: query tile 7 - w done
#ifdef VAPX_TRACE
  if (a.trace && tid == 0 && blockIdx.x < 16384) { a.trace[(long)blockIdx.x * 32 + 29] = __builtin_amdgcn_s_memrealtime(); a.trace[(long)blockIdx.x * 32 + 30] = (unsigned long long)stamp_k; }
#endif
}

// ------------------------------------------------------------------------------------------------
// 4a'. windows of 257 .. 512 frames (round 5).  The reference's ALiBi transformer takes any T (modules.py:303-308: the mask is rebuilt
//      for the sequence at hand); no published checkpoint goes beyond 10 s x 20 Hz = 200 frames, so this kernel is the plain form of the
//      one above, built to be right rather than tuned: one workgroup per (stream, channel, head), four waves, wave w takes the query
//      tiles w, 7 - w, 8 + w, 15 - w (balanced); K fragments AND the V rows come straight from global / L2 (512 keys x 64 features would be 128 KB
//      of LDS), the softmax is online per 32-key tile exactly as above.  Same operand layouts, same masking, same arithmetic order per
//      tile — a window of <= 256 frames run through this kernel gives attention_long2_kernel's results (tests/test_engine_gpu.py).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attention_xl_kernel(AttnArgs a) {
  const int T = a.T;
  const int n_tiles = (T + 31) >> 5;                 // <= 16
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = (int)(blockIdx.x & 3), bc = (int)(blockIdx.x >> 2), b = bc >> 1;
  const int n = a.bn[b];
  const int kvbc = a.swap_kv ? (bc ^ 1) : bc;
  const int l31 = lane & 31, hi = lane >> 5;
  const bool ringed = a.ring_rot != nullptr;
  const int rot = ringed ? a.ring_rot[b] : 0;
  const long slab_q = ringed ? ((long)(a.ids ? a.ids[b] : b) * 2 + (bc & 1)) : (long)bc;
  const long slab_kv = ringed ? slab_q : (long)kvbc;
  auto prow = [&](int i) { int r = i + rot; return r >= T ? r - T : r; };
  const float* kp = a.k + slab_kv * T * a.ldkv + h * 64;
  const float* vp = a.v + slab_kv * T * a.ldkv + h * 64;
  const int nt_valid = (n + 31) >> 5;
  const float slope = exp2f(-2.0f * (float)(h + 1));  // [1/4, 1/16, 1/64, 1/256]
  const float hi4f = (float)(4 * hi);
  for (int pass = 0; pass < 4; ++pass) {
    const int it = pass * 4 + ((pass & 1) ? 3 - w : w);   // zig-zag over the waves: 34 causal key tiles for every wave of a full 512-frame window
    if (it >= n_tiles) continue;
    const int i = it * 32 + l31;
    float* op = a.out + ((long)bc * T + i) * 256 + h * 64;
    if (it >= nt_valid) {                             // whole tile beyond the valid rows: deterministic zeros
      if (i < T)
#pragma unroll
        for (int d = 0; d < 8; ++d) *(f32x4*)(op + hi * 32 + d * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    f32x4 qf[8];
    {
      const int ic = i < n ? i : n - 1;
      const float* qp = a.q + (slab_q * T + prow(ic)) * a.ldq + h * 64 + hi * 4;
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) qf[kc] = *(const f32x4*)(qp + kc * 8);
    }
    float m = -1e30f, l = 0.f;
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
#pragma unroll 1
    for (int jt = 0; jt <= it; ++jt) {
      f32x4 kf[8];
      {
        int j = jt * 32 + l31;
        j = j < n ? j : n - 1;                         // rows beyond the window: clamped, masked below
        const float* kr = kp + (long)prow(j) * a.ldkv + hi * 4;
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) kf[kc] = *(const f32x4*)(kr + kc * 8);
      }
      float v0[16], v1[16];                            // V^T operands of the 16 MFMA steps: key 32 jt + C_r + 4 hi, features l31 and l31 + 32
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        j = j < n ? j : n - 1;                         // (its P is exactly 0)
        const float* va = vp + (long)prow(j) * a.ldkv + l31;
        v0[r] = va[0]; v1[r] = va[32];
      }
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < 8; ++kc)
#pragma unroll
        for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[kc][s], qf[kc][s], sc, 0, 0, 0);
      float cm = -1e30f;
      const float jb = (float)(jt * 32) + hi4f;
      const int i4 = i - jt * 32 - 4 * hi, n4 = n - jt * 32 - 4 * hi;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2);
        float v = fmaf(sc[r], 0.0625f, slope * ((float)c + jb));
        v = ((c <= i4) && (c < n4)) ? v : -1e30f;
        sc[r] = v;
        cm = fmaxf(cm, v);
      }
      cm = fmaxf(cm, __shfl_xor(cm, 32));
      const float mn = fmaxf(m, cm);
      const float alpha = __expf(m - mn);
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pr = sc[r] > -1e29f ? __expf(sc[r] - mn) : 0.f;
        sc[r] = pr;
        sum += pr;
      }
      sum += __shfl_xor(sum, 32);
      l = l * alpha + sum;
      m = mn;
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[r], sc[r], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[r], sc[r], o1, 0, 0, 0);
      }
    }
    if (i < T) {
      const float scl = i < n ? 1.0f / l : 0.f;         // rows beyond the valid window: deterministic zeros
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        f32x4 x0 = {o0[rr * 4 + 0], o0[rr * 4 + 1], o0[rr * 4 + 2], o0[rr * 4 + 3]};
        f32x4 x1 = {o1[rr * 4 + 0], o1[rr * 4 + 1], o1[rr * 4 + 2], o1[rr * 4 + 3]};
        *(f32x4*)(op + rr * 8 + hi * 4) = x0 * scl;
        *(f32x4*)(op + 32 + rr * 8 + hi * 4) = x1 * scl;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 4b. last-row path of the final layer.  Only the newest row of the last stereo layer reaches the
//     heads (vap_main.py:316-317 takes [-1]); its K/V still need every row, but Q, the attention
//     output, both projections and the FFN are needed for ONE row per (stream, channel).  Exact.
// ------------------------------------------------------------------------------------------------
// gather row n-1 of every (stream, channel) and LayerNorm it: one wave per (b,c)
__global__ __launch_bounds__(256) void gather_last_ln_kernel(LastRowArgs a) {
  const int lane = threadIdx.x & 63;
  const int bc = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bc >= a.B * 2) return;
  const int n = a.bn[bc >> 1];
  f32x4 v = *(const f32x4*)(a.x + ((long)bc * a.T + n - 1) * 256 + lane * 4);
  *(f32x4*)(a.xlast + (long)bc * 256 + lane * 4) = v;
  float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
  f32x4 d = v - mean;
  float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 256.0f);
  float rstd = rsqrtf(var + 1e-5f);
  f32x4 g = *(const f32x4*)(a.gamma + lane * 4), be = *(const f32x4*)(a.beta + lane * 4);
  *(f32x4*)(a.xnlast + (long)bc * 256 + lane * 4) = d * rstd * g + be;
}

// LayerNorm of plain [rows][256] rows, one wave per row (trunk followers: en = LN0(e))
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, int rows) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  f32x4 v = *(const f32x4*)(x + (long)r * 256 + lane * 4);
  float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
  f32x4 d = v - mean;
  float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 256.0f);
  float rstd = rsqrtf(var + 1e-5f);
  f32x4 g = *(const f32x4*)(gamma + lane * 4), be = *(const f32x4*)(beta + lane * 4);
  *(f32x4*)(y + (long)r * 256 + lane * 4) = d * rstd * g + be;
}

// single-query attention: query = newest row (index n-1, so every key j < n is causal-visible),
// one workgroup per (stream, channel), one wave per head.  Phase 1: lane = key j computes the
// score; softmax across lanes; phase 2: lane = feature d accumulates sum_j p_j V[j][d].
__global__ __launch_bounds__(256) void attention_last_kernel(AttnArgs a) {
  const int bc = blockIdx.x, b = bc >> 1, h = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = a.bn[b], T = a.T;
  const int kvbc = a.swap_kv ? (bc ^ 1) : bc;
  const float qm = a.q[(long)bc * a.ldq + h * 64 + lane] * 0.0625f;   // element `lane` of this head's query; broadcast from registers
  const float slope = exp2f(-2.0f * (float)(h + 1));
  const float* kp = a.k + (long)kvbc * T * a.ldkv + h * 64;
  const float* vp = a.v + (long)kvbc * T * a.ldkv + h * 64;
  float mx = -1e30f, l = 0.f, o = 0.f;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    float sc = -1e30f;
    if (j < n) {
      const f32x4* kr = (const f32x4*)(kp + (long)j * a.ldkv);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 16; ++c)
        acc += kr[c] * f32x4{lane_bcast(qm, c * 4), lane_bcast(qm, c * 4 + 1), lane_bcast(qm, c * 4 + 2), lane_bcast(qm, c * 4 + 3)};
      sc = (acc[0] + acc[1]) + (acc[2] + acc[3]) + slope * (float)j;
    }
    const float mn = fmaxf(mx, wave_max(sc));
    const float pj = j < n ? expf(sc - mn) : 0.f;
    const float corr = expf(mx - mn);
    l = l * corr + wave_sum(pj);
    o *= corr;
    mx = mn;
    const int jn = (n - j0) < 64 ? (n - j0) : 64;
    for (int jj = 0; jj < jn; ++jj) o += lane_bcast(pj, jj) * vp[(long)(j0 + jj) * a.ldkv + lane];   // p_j from registers (no LDS)
  }
  a.out[(long)bc * 256 + h * 64 + lane] = o / l;
}

// ------------------------------------------------------------------------------------------------
// 5. Combinator + heads on the newest row of each stream
//    reference: Combinator.forward modules.py:449-464; vap_head / va_classifier / softmax
//    vap_main.py:290-295,313-314; probs_next_speaker_aggregate objective.py:186-206;
//    bc / nod heads vap_bc_main.py:272-277, vap_nod_main.py:273-279.
//    HB (2 or 4) streams per workgroup; thread j owns output feature j (weights pre-transposed [k][j] so
//    the 256 threads read one coalesced row per k); row-wise reductions via wave butterflies +
//    one LDS exchange.
// ------------------------------------------------------------------------------------------------

// Cross-wave exchange of N per-wave values through LDS.  No thread reads LDS with a wave-uniform address: on this MI355X pool a
// wave-uniform ds_read_b128 returns wrong data when ANOTHER wave on the CU runs K=16 f16 / bf16 MFMAs (another engine with
// VAPX_FLAG_SPLIT_F16, another process; reproducer: tools/mfma_victim + tools/mfma_aggr, DESIGN.md "co-running f16 MFMA").
// Every lane fetches one distinct word and the values are broadcast from registers (v_readlane).  4 N <= 64.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float* red /* [64] */, int wave, int lane) {
  static_assert(4 * N <= 64, "one word per lane");
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
  __syncthreads();
  const float mine = red[lane];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = lane_bcast(mine, i) + lane_bcast(mine, N + i) + lane_bcast(mine, 2 * N + i) + lane_bcast(mine, 3 * N + i);
}
template <int N>
__device__ __forceinline__ void block_max(float (&v)[N], float* red, int wave, int lane) {
  static_assert(4 * N <= 64, "one word per lane");
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_max(v[i]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
  __syncthreads();
  const float mine = red[lane];
#pragma unroll
  for (int i = 0; i < N; ++i)
    v[i] = fmaxf(fmaxf(lane_bcast(mine, i), lane_bcast(mine, N + i)), fmaxf(lane_bcast(mine, 2 * N + i), lane_bcast(mine, 3 * N + i)));
}

// y[s][j] = sum_k WT[k][j] * x[s][k] for the HB streams of the block: the k range is split over the 4
// waves (64 k each), each lane accumulates 4 adjacent outputs with 16-byte weight loads (a 1 KiB
// coalesced row per wave instruction), partials are combined through LDS.  Thread j returns y[.][j].
// xm[s] = x[s][j]: thread j = 64 w + lane holds exactly element `lane` of its wave's k slice, so the
// activations are broadcast from registers (v_readlane) and never staged in LDS.
template <int HB>
__device__ __forceinline__ void block_matvec(const float* __restrict__ WT, const float (&xm)[HB], float* psum /* [4][HB][256] */,
                                             float (&y)[HB], int j) {
  const int lane = j & 63, w = j >> 6;
  f32x4 part[HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) part[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wp = WT + (long)(w * 64) * 256 + lane * 4;
#pragma unroll
  for (int kk = 0; kk < 64; kk += 4) {
    f32x4 wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wv[u] = *(const f32x4*)(wp + (long)(kk + u) * 256);
#pragma unroll
    for (int s = 0; s < HB; ++s)
#pragma unroll
      for (int u = 0; u < 4; ++u) part[s] += wv[u] * lane_bcast(xm[s], kk + u);
  }
  __syncthreads();   // psum may still be read from a previous call
#pragma unroll
  for (int s = 0; s < HB; ++s) *(f32x4*)&psum[(w * HB + s) * 256 + lane * 4] = part[s];
  __syncthreads();
#pragma unroll
  for (int s = 0; s < HB; ++s)
    y[s] = (psum[(0 * HB + s) * 256 + j] + psum[(1 * HB + s) * 256 + j]) + (psum[(2 * HB + s) * 256 + j] + psum[(3 * HB + s) * 256 + j]);
}

template <int HB>
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float psum[4 * HB * 256];
  __shared__ float red[64];
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int b0 = blockIdx.x * HB;
  int nb[HB];
  float xa[HB], xb[HB];   // newest rows of the two towers, element j
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    int b = b0 + s;
    b = b < a.B ? b : a.B - 1;
    nb[s] = a.bn[b];
    xa[s] = a.x_last_only ? a.x[((long)b * 2) * 256 + j] : a.x[(((long)b * 2) * a.T + nb[s] - 1) * 256 + j];
    xb[s] = a.x_last_only ? a.x[((long)b * 2 + 1) * 256 + j] : a.x[(((long)b * 2 + 1) * a.T + nb[s] - 1) * 256 + j];
  }
  // combinator projections
  float ha[HB], hb[HB];
  block_matvec<HB>(a.waT, xa, psum, ha, j);
  block_matvec<HB>(a.wbT, xb, psum, hb, j);
  // shared LayerNorm on both, exact GELU, sum
  float v[2 * HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) { v[2 * s] = ha[s]; v[2 * s + 1] = hb[s]; }
  block_sum<2 * HB>(v, red, wave, lane);
  float mean[2 * HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    mean[2 * s] = v[2 * s] * (1.0f / 256.0f);
    mean[2 * s + 1] = v[2 * s + 1] * (1.0f / 256.0f);
    float da = ha[s] - mean[2 * s], db = hb[s] - mean[2 * s + 1];
    v[2 * s] = da * da;
    v[2 * s + 1] = db * db;
  }
  block_sum<2 * HB>(v, red, wave, lane);
  const float cg = a.cg[j], cb = a.cb[j];
  float hs[HB];   // combinator output, element j
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    float ya = (ha[s] - mean[2 * s]) * rsqrtf(v[2 * s] * (1.0f / 256.0f) + 1e-5f) * cg + cb;
    float yb = (hb[s] - mean[2 * s + 1]) * rsqrtf(v[2 * s + 1] * (1.0f / 256.0f) + 1e-5f) * cg + cb;
    hs[s] = gelu_erf(ya) + gelu_erf(yb);
  }
  // vap_head logits
  float lg[HB];
  block_matvec<HB>(a.hwT, hs, psum, lg, j);
  const float hbias = a.hb[j];
#pragma unroll
  for (int s = 0; s < HB; ++s) lg[s] += hbias;
  float mxv[HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) mxv[s] = lg[s];
  block_max<HB>(mxv, red, wave, lane);
  float ex[HB], den[HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) { ex[s] = expf(lg[s] - mxv[s]); den[s] = ex[s]; }
  block_sum<HB>(den, red, wave, lane);
  // class j <-> 8 bits; channel c bins = bits 4c..4c+3; now = bins 0-1, future = bins 2-3
  const float n0w = (float)((j & 1) + ((j >> 1) & 1)), n1w = (float)(((j >> 4) & 1) + ((j >> 5) & 1));
  const float f0w = (float)(((j >> 2) & 1) + ((j >> 3) & 1)), f1w = (float)(((j >> 6) & 1) + ((j >> 7) & 1));
  float pn0[HB], pn1[HB], pf0[HB], pf1[HB];
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    float p = ex[s] / den[s];
    pn0[s] = p * n0w; pn1[s] = p * n1w; pf0[s] = p * f0w; pf1[s] = p * f1w;
  }
  block_sum<HB>(pn0, red, wave, lane);
  block_sum<HB>(pn1, red, wave, lane);
  block_sum<HB>(pf0, red, wave, lane);
  block_sum<HB>(pf1, red, wave, lane);
  // VAD on the ar_channel outputs (note: o, not the stereo towers)  vap_main.py:292-293
  float vd[2 * HB];
  const float vw = a.vw[j];
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    int b = b0 + s;
    b = b < a.B ? b : a.B - 1;
#pragma unroll
    for (int c = 0; c < 2; ++c) vd[2 * s + c] = vw * a.o[(((long)b * 2 + c) * a.T + nb[s] - 1) * 256 + j];
  }
  block_sum<2 * HB>(vd, red, wave, lane);
  // auxiliary heads (bc: rows 0..2 softmax; nod: rows 0..3 softmax)
  float ax[4][HB];
  if (a.mode != 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float wr = a.aw[r * 256 + j];
#pragma unroll
      for (int s = 0; s < HB; ++s) ax[r][s] = wr * hs[s];
      block_sum<HB>(ax[r], red, wave, lane);
    }
  }
#pragma unroll
  for (int s = 0; s < HB; ++s) {
    int b = b0 + s;
    if (b >= a.B) break;
    float* out = a.out + (long)b * a.out_stride;
    out[16 + j] = lg[s];
    out[272 + j] = a.e[((long)b * 2) * 256 + j];
    out[272 + 256 + j] = a.e[((long)b * 2 + 1) * 256 + j];
    if (j == 0) {
      float dn = pn0[s] + pn1[s] + 1e-5f, df = pf0[s] + pf1[s] + 1e-5f;
      out[0] = pn0[s] / dn; out[1] = pn1[s] / dn;
      out[2] = pf0[s] / df; out[3] = pf1[s] / df;
      out[4] = sigmoidf_(vd[2 * s] + a.vb[0]);
      out[5] = sigmoidf_(vd[2 * s + 1] + a.vb[0]);
      out[11] = vd[2 * s] + a.vb[0];          // va_classifier outputs before the sigmoid (VapGPT.forward returns these)
      out[12] = vd[2 * s + 1] + a.vb[0];
      out[10] = (float)nb[s];
      out[14] = 0.f; out[15] = 0.f;            // reserved slots: the whole row is defined, whatever the buffer held before
      if (a.mode == 0) { out[6] = 0.f; out[7] = 0.f; out[8] = 0.f; out[9] = 0.f; }
      if (a.mode != 0) {
        int nr = a.mode == 1 ? 3 : 4;
        float z[4], zm = -1e30f, zs = 0.f;
        for (int r = 0; r < nr; ++r) { z[r] = ax[r][s] + a.ab[r]; zm = fmaxf(zm, z[r]); }
        for (int r = 0; r < nr; ++r) { z[r] = expf(z[r] - zm); zs += z[r]; }
        for (int r = 0; r < 4; ++r) out[6 + r] = r < nr ? z[r] / zs : 0.f;
      }
      {   // per-row numeric status (VAPX_OUT_STATUS): 1 = p_now / p_future / VAD / aux probabilities not all finite (poisoned state)
        float chk = (out[0] + out[1]) + (out[2] + out[3]) + (out[4] + out[5]);
        if (a.mode != 0) chk += (out[6] + out[7]) + (out[8] + out[9]);
        out[13] = (chk - chk == 0.f) ? 0.f : 1.f;
      }
      if (a.frames_seen) {
        int sid = a.ids ? a.ids[b] : b;
        int fs = a.frames_seen[sid] + 1;
        // only fs % T and min(fs, T) are ever used: fold the counter long before it could overflow (2^30 frames = 1.7 years at 20 Hz)
        if (fs >= (1 << 30)) fs = a.T + fs % a.T;
        a.frames_seen[sid] = fs;
      }
    }
  }
}

// Wire rows of a trunk group's tick (vapx_step_group): the first wf floats of every model's [n][VAPX_OUT_STRIDE] output rows, packed
// model-major into one block [model m][n][wf(m)] that a single linear copy takes to the host.  One 16-byte load and one 16-byte
// store per lane; blockIdx.y = model.  Rows are 16-byte aligned on both sides (784 and every wf are multiples of 4 floats).
__global__ __launch_bounds__(256) void wire_pack_kernel(WirePackArgs a) {
  const int m = blockIdx.y;
  const int wf4 = a.wf4[m];
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.n * wf4) return;
  const long row = idx / wf4;
  const int q = (int)(idx - row * wf4);
  const f32x4 v = *(const f32x4*)(a.src[m] + row * a.src_stride + q * 4);
  *(f32x4*)(a.dst + a.dst_off[m] + idx * 4) = v;
}

// Trunk follower at 1/R of its leader's rate: a pure copy keyed by STREAM ID (batches are ragged and reorder between ticks).  One
// workgroup per (entry, channel); a wave moves a row of 256 floats with one 16-byte load and store per lane.  A due entry k gets the
// follower's downsample operand A[k][c] = the stream's (R-1) * ncpc_l collected rows followed by this tick's ncpc_l leader rows, and
// its window fill / ring slot from the follower's own frame counter; a not-due entry parks this tick's rows in the stream's acc.
__global__ __launch_bounds__(256) void trunk_collect_kernel(TrunkCollectArgs a) {
  const int k = blockIdx.x, c = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sid = a.sid[k], slot = a.slot[k];
  const int nl = a.ncpc_l, na = (a.R - 1) * nl;
  const float* src = a.lstm_out + ((long)slot * 2 + c) * nl * 256 + lane * 4;
  float* accp = a.acc + ((long)sid * 2 + c) * na * 256 + lane * 4;
  if (k < a.n_due) {
    float* dst = a.A + ((long)k * 2 + c) * (na + nl) * 256 + lane * 4;
    for (int r = w; r < na + nl; r += 4)
      *(f32x4*)(dst + (long)r * 256) = r < na ? *(const f32x4*)(accp + (long)r * 256) : *(const f32x4*)(src + (long)(r - na) * 256);
    if (c == 0 && threadIdx.x == 0) {
      const int fs = a.frames_seen[sid];
      a.bn[k] = fs + 1 < a.T ? fs + 1 : a.T;
      a.bhead[k] = fs % a.T;
    }
  } else {
    float* dst = accp + (long)a.pos[k] * nl * 256;
    for (int r = w; r < nl; r += 4) *(f32x4*)(dst + (long)r * 256) = *(const f32x4*)(src + (long)r * 256);
  }
}

// The follower's compact rows back into the leader's batch order; a stream without a frame this tick gets an all-zero row whose
// VAPX_OUT_STATUS is VAPX_STATUS_NO_FRAME (2).  One workgroup per entry, one 16-byte store per lane.
__global__ __launch_bounds__(256) void out_scatter_kernel(OutScatterArgs a) {
  const int k = blockIdx.x, q = threadIdx.x;
  if (q * 4 >= a.stride) return;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (k < a.n_due) v = *(const f32x4*)(a.src + (long)k * a.stride + q * 4);
  else if (q == 3) v[1] = 2.f;   // float 13
  *(f32x4*)(a.dst + (long)a.slot[k] * a.stride + q * 4) = v;
}

__global__ void window_meta_kernel(const int* ids, const int* frames_seen, int T, int* bn, int* bhead, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int fs = frames_seen[ids ? ids[i] : i];
  bn[i] = fs + 1 < T ? fs + 1 : T;
  bhead[i] = fs % T;
}

}  // namespace

hipError_t launch_conv0(const Conv0Args& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(conv0_kernel, dim3(B * 2), dim3(256), a.L * sizeof(float), st, a);
  return hipGetLastError();
}
hipError_t launch_lstm(const LstmArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(lstm_kernel, dim3((a.M + 15) / 16), dim3(512), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_conv0_prefill(const Conv0PrefillArgs& a, int V, hipStream_t st) {
  hipLaunchKernelGGL(conv0_kernel, dim3(V * 2), dim3(256), a.L * sizeof(float), st, a);
  return hipGetLastError();
}
hipError_t launch_lstm_prefill(const LstmPrefillArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(lstm_kernel, dim3((a.M + 15) / 16), dim3(512), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_prefill_fill(const PrefillFillArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ring_append_kernel, dim3((a.fc * a.n * 2 + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_ring_append(const GatherArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(ring_append_kernel, dim3((a.B * 2 + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_gather_ln(const GatherArgs& a, hipStream_t st) {
  long rows = (long)a.B * 2 * a.T;
  hipLaunchKernelGGL(gather_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_attention(const AttnArgs& a, int B, hipStream_t st, bool force_xl) {
  const int n_tiles = (a.T + 31) / 32;
  if (n_tiles > 16) return hipErrorInvalidValue;         // T <= 512 (vapx_create enforces it)
  if (n_tiles > 8 || force_xl) {   // 257 .. 512 frames (force_xl: the engine's VAPX_FORCE_ATTENTION_XL, tests hold the kernel against attention_long2_kernel)
    hipLaunchKernelGGL(attention_xl_kernel, dim3(B * 2 * 4), dim3(256), 0, st, a);
    return hipGetLastError();
  }
  static PerDeviceOnce attr_set;
  attr_set.run([] { (void)hipFuncSetAttribute((const void*)attention_long2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024); });
  hipLaunchKernelGGL(attention_long2_kernel, dim3(B * 2 * 4), dim3(256), (size_t)n_tiles * 32 * 64 * sizeof(float), st, a);
  return hipGetLastError();
}
hipError_t launch_gather_last_ln(const LastRowArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(gather_last_ln_kernel, dim3((a.B * 2 + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_ln_rows(const float* x, float* y, const float* gamma, const float* beta, int rows, hipStream_t st) {
  hipLaunchKernelGGL(ln_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, y, gamma, beta, rows);
  return hipGetLastError();
}
hipError_t launch_attention_last(const AttnArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(attention_last_kernel, dim3(B * 2), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_head(const HeadArgs& a, hipStream_t st) {
  // streams per workgroup: every workgroup streams the same 0.8 MB of weights, so few streams per workgroup spread a small
  // batch over more CUs (2: 30 us at 256 streams vs 56 us with 8), more amortise the stream at large batches
  if (a.B <= 1024) hipLaunchKernelGGL(head_kernel<2>, dim3((a.B + 1) / 2), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(head_kernel<4>, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_wire_pack(const WirePackArgs& a, hipStream_t st) {
  int wmax = 0;
  for (int m = 0; m < a.n_models; ++m) wmax = a.wf4[m] > wmax ? a.wf4[m] : wmax;
  const long items = (long)a.n * wmax;
  hipLaunchKernelGGL(wire_pack_kernel, dim3((unsigned)((items + 255) / 256), a.n_models), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_trunk_collect(const TrunkCollectArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(trunk_collect_kernel, dim3(a.n, 2), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_out_scatter(const OutScatterArgs& a, hipStream_t st) {
  if (a.stride > 1024 || a.stride % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(out_scatter_kernel, dim3(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_window_meta(const int* ids, const int* frames_seen, int T, int* bn, int* bhead, int n, hipStream_t st) {
  hipLaunchKernelGGL(window_meta_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ids, frames_seen, T, bn, bhead, n);
  return hipGetLastError();
}
