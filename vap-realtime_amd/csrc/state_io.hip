// Stream-state export / import: vapx_export_streams / vapx_import_streams (include/vapx.h "Bulk state export / import") and, one stream
// at a time through an engine-internal record, vapx_get_state / vapx_set_state.  The record's layout is state_record.h's.
// Pure data movement: no LDS, no atomics, every access a plain 16-byte vector load / store.  One wave moves one 256-float ring row
// (64 lanes x 16 bytes, coalesced on both sides) and, when the cache travels, the row's three 256-float Q | K | V segments with it: four
// independent 16-byte loads in flight per lane before the first store.  A workgroup is four such waves; the grid is
// (items / 4, streams) with 2T row items + 9 small ones (4 LSTM rows, 3 carry chunks, the header, the resampler history of an engine with an input rate) per stream, so the C3 shape
// (4096 streams, T = 250) is half a million workgroups of 16 KiB each: the chip is oversubscribed many times over and the only limit is HBM.
#include <hip/hip_runtime.h>

#include "vap_kernels.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kHeaderItem = 7, kResampleItem = 8;
constexpr int kSmallItems = 9;                              // 4 LSTM rows, 3 carry chunks (640 floats = 2.5 rows), 1 header, 1 resampler history
constexpr int kMaxGridY = 32768;
static_assert(kStateLstmFloats == 4 * 256 && kStateCarryFloats == 2 * VAPX_PAD, "state_record.h against the small items and common.h");

// export: ring slot ((fs - n + t) mod T) -> chronological row t, zero rows beyond n = min(fs, T)
__global__ __launch_bounds__(256) void state_export_kernel(StateIoArgs a) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int T = a.T, k = blockIdx.y;
  if (item >= 2 * T + kSmallItems) return;
  const int sid = a.ids ? a.ids[k] : a.id0 + k;
  const int fs = a.frames_seen[sid];
  const int nn = fs < 0 ? 0 : (fs < T ? fs : T);
  const StateLayout& L = a.lay;
  float* r = a.rec + (long)k * L.total;
  if (item < 2 * T) {
    if (!(a.sections & SEC_RING)) return;
    const bool cache = a.sections & SEC_CACHE;
    const int c = item >= T ? 1 : 0, t = item - c * T;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    f32x4 q0 = v, q1 = v, q2 = v;
    if (t < nn) {
      const int slot = (fs - nn + t) % T;
      const long srow = ((long)sid * 2 + c) * T + slot;
      v = *(const f32x4*)(a.ring + srow * 256 + lane * 4);
      if (cache) {
        const float* qs = a.ring_qkv + srow * 768 + lane * 4;
        q0 = *(const f32x4*)(qs); q1 = *(const f32x4*)(qs + 256); q2 = *(const f32x4*)(qs + 512);
      }
    }
    *(f32x4*)(r + L.ring + (long)item * 256 + lane * 4) = v;
    if (cache) {
      float* qd = r + L.cache + (long)item * 768 + lane * 4;
      *(f32x4*)(qd) = q0; *(f32x4*)(qd + 256) = q1; *(f32x4*)(qd + 512) = q2;
    }
    return;
  }
  const int j = item - 2 * T;
  if (j == kHeaderItem) {
    if (lane == 0) *(i32x4*)(r + L.header) = i32x4{a.hdr[SH_MAGIC], a.hdr[SH_CTX_FRAMES], a.hdr[SH_FRAME_HZ], a.hdr[SH_BITS]};
    if (lane == 1) {
      const int st = a.rs_started ? (a.rs_started[sid * 2] != 0) | ((a.rs_started[sid * 2 + 1] != 0) << 1) : 0;
      *(i32x4*)(r + L.header + SH_N_FRAMES) = i32x4{nn, a.hdr[SH_MODE], a.hdr[SH_INPUT_HZ], st};
    }
  } else if (j == kResampleItem) {     // history [2][H] + padding
    if ((a.sections & SEC_HISTORY) && lane * 4 < a.rs_rec)
      *(f32x4*)(r + L.history + lane * 4) = *(const f32x4*)(a.rs_hist + (long)sid * a.rs_rec + lane * 4);
  } else if (j < 4) {         // record lstm [ch][(h, c)][256]  <-  h_state / c_state [S*2][256]
    if (!(a.sections & SEC_LSTM)) return;
    const float* src = ((j & 1) ? a.c_state : a.h_state) + ((long)sid * 2 + (j >> 1)) * 256;
    *(f32x4*)(r + L.lstm + j * 256 + lane * 4) = *(const f32x4*)(src + lane * 4);
  } else {                             // carry [2][320]: 160 16-byte pieces over three waves
    const int q = (j - 4) * 64 + lane;
    if ((a.sections & SEC_CARRY) && q < kStateCarryFloats / 4)
      *(f32x4*)(r + L.carry + q * 4) = *(const f32x4*)(a.carry + (long)sid * kStateCarryFloats + q * 4);
  }
}

// import: chronological row t -> ring slot t (t < n_frames, clamped into [0, T]); frames_seen = n_frames.  Only what a.sections names
__global__ __launch_bounds__(256) void state_import_kernel(StateIoArgs a) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int T = a.T, k = blockIdx.y;
  if (item >= 2 * T + kSmallItems) return;
  const int sid = a.ids ? a.ids[k] : a.id0 + k;
  const StateLayout& L = a.lay;
  const float* r = a.rec + (long)k * L.total;
  const int* hd = (const int*)(r + L.header);
  int nn = hd[SH_N_FRAMES];
  nn = nn < 0 ? 0 : (nn < T ? nn : T);
  if (item < 2 * T) {
    const int c = item >= T ? 1 : 0, t = item - c * T;
    if (!(a.sections & SEC_RING) || t >= nn) return;
    const long drow = ((long)sid * 2 + c) * T + t;
    const f32x4 v = *(const f32x4*)(r + L.ring + (long)item * 256 + lane * 4);
    if (a.sections & SEC_CACHE) {
      const float* qs = r + L.cache + (long)item * 768 + lane * 4;
      const f32x4 q0 = *(const f32x4*)(qs), q1 = *(const f32x4*)(qs + 256), q2 = *(const f32x4*)(qs + 512);
      float* qd = a.ring_qkv + drow * 768 + lane * 4;
      *(f32x4*)(qd) = q0; *(f32x4*)(qd + 256) = q1; *(f32x4*)(qd + 512) = q2;
    }
    *(f32x4*)(a.ring + drow * 256 + lane * 4) = v;
    return;
  }
  const int j = item - 2 * T;
  if (j == kHeaderItem) {
    if (lane == 0 && (a.sections & SEC_RING)) a.frames_seen[sid] = nn;
    if (lane < 2 && a.rs_started) a.rs_started[sid * 2 + lane] = (hd[SH_STARTED] >> lane) & 1;
  } else if (j == kResampleItem) {
    if ((a.sections & SEC_HISTORY) && lane * 4 < a.rs_rec)
      *(f32x4*)(a.rs_hist + (long)sid * a.rs_rec + lane * 4) = *(const f32x4*)(r + L.history + lane * 4);
  } else if (j < 4) {
    if (!(a.sections & SEC_LSTM)) return;
    float* dst = ((j & 1) ? a.c_state : a.h_state) + ((long)sid * 2 + (j >> 1)) * 256;
    *(f32x4*)(dst + lane * 4) = *(const f32x4*)(r + L.lstm + j * 256 + lane * 4);
  } else {
    const int q = (j - 4) * 64 + lane;
    if ((a.sections & SEC_CARRY) && q < kStateCarryFloats / 4)
      *(f32x4*)(a.carry + (long)sid * kStateCarryFloats + q * 4) = *(const f32x4*)(r + L.carry + q * 4);
  }
}

// LayerNorm(ln_self of layer 0) of every ring row of the chunk's streams, one wave per row (the arithmetic of gather_ln_kernel)
__global__ __launch_bounds__(256) void state_ln_kernel(const float* __restrict__ ring, const int* __restrict__ ids, int id0,
                                                       float* __restrict__ xn, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int T, int n) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)n * 2 * T) return;
  const int k = (int)(row / (2 * T)), rem = (int)(row - (long)k * 2 * T);
  const int sid = ids ? ids[k] : id0 + k;
  f32x4 v = *(const f32x4*)(ring + ((long)sid * 2 * T + rem) * 256 + lane * 4);
  float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.0f / 256.0f);
  f32x4 d = v - mean;
  float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 256.0f);
  float rstd = rsqrtf(var + 1e-5f);
  f32x4 g = *(const f32x4*)(gamma + lane * 4), be = *(const f32x4*)(beta + lane * 4);
  *(f32x4*)(xn + row * 256 + lane * 4) = d * rstd * g + be;
}

// rebuilt cache rows [n][2][T][768] -> the streams' cache slots; rows beyond the window fill stay as they were (never read)
__global__ __launch_bounds__(256) void state_cache_scatter_kernel(const float* __restrict__ qkv, const int* __restrict__ ids, int id0,
                                                                  float* __restrict__ ring_qkv, const int* __restrict__ frames_seen,
                                                                  int T, int n) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)n * 2 * T) return;
  const int k = (int)(row / (2 * T)), rem = (int)(row - (long)k * 2 * T);
  const int sid = ids ? ids[k] : id0 + k;
  const int t = rem >= T ? rem - T : rem;
  if (t >= frames_seen[sid]) return;
  const float* qs = qkv + row * 768 + lane * 4;
  const f32x4 q0 = *(const f32x4*)(qs), q1 = *(const f32x4*)(qs + 256), q2 = *(const f32x4*)(qs + 512);
  float* qd = ring_qkv + ((long)sid * 2 * T + rem) * 768 + lane * 4;
  *(f32x4*)(qd) = q0; *(f32x4*)(qd + 256) = q1; *(f32x4*)(qd + 512) = q2;
}

template <typename K>
hipError_t launch_per_stream(K kernel, StateIoArgs a, hipStream_t st) {
  const unsigned gx = (unsigned)((2 * a.T + kSmallItems + 3) / 4);
  const int n = a.n;
  for (int k0 = 0; k0 < n; k0 += kMaxGridY) {   // gridDim.y is a 16-bit quantity
    StateIoArgs c = a;
    c.n = n - k0 < kMaxGridY ? n - k0 : kMaxGridY;
    c.rec = a.rec + (long)k0 * a.lay.total;
    if (a.ids) c.ids = a.ids + k0; else c.id0 = a.id0 + k0;
    hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)c.n), dim3(256), 0, st, c);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_state_export(const StateIoArgs& a, hipStream_t st) { return launch_per_stream(state_export_kernel, a, st); }
hipError_t launch_state_import(const StateIoArgs& a, hipStream_t st) { return launch_per_stream(state_import_kernel, a, st); }

hipError_t launch_state_ln(const float* ring, const int* ids, int id0, float* xn, const float* gamma, const float* beta, int T, int n,
                           hipStream_t st) {
  const long rows = (long)n * 2 * T;
  hipLaunchKernelGGL(state_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, ring, ids, id0, xn, gamma, beta, T, n);
  return hipGetLastError();
}

hipError_t launch_state_cache_scatter(const float* qkv, const int* ids, int id0, float* ring_qkv, const int* frames_seen, int T, int n,
                                      hipStream_t st) {
  const long rows = (long)n * 2 * T;
  hipLaunchKernelGGL(state_cache_scatter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, qkv, ids, id0, ring_qkv, frames_seen, T, n);
  return hipGetLastError();
}
