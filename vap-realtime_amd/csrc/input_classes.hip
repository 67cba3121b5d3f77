// The engine's one input path: whatever the caller's audio is, input_classes_kernel turns a tick's block into the 16 kHz fp32 rows conv0
// takes, in one launch.  A class is (format, rate).  An engine with a table (vapx_set_input_classes; include/vapx.h "Input classes") gives
// every (stream, channel) a class of its own; its tick is a packed block in which batch slot k holds a row per channel, described
// by slot descriptors the host builds.  A uniform engine (vapx_set_input_rate and / or vapx_set_input_format) is a table of ONE class with
// no descriptors: slot b is class 0 at b x (bytes of its two rows), computed here.
// One 256-thread workgroup per (batch slot, channel).  With a table a class belongs to a (stream, channel): the slot holds channel 1's row
// of its class, then channel 2's of its own, and the two workgroups of a slot may take different paths.  A workgroup's class is uniform
// over it; its geometry is read once from the kernel arguments and lives in scalars.
//   - load + decode: lane i reads the aligned dword at the row's base + 4 i (four G.711 codes, two s16 samples or one float) and expands
//     it with the device functions of input_decode.h, the ones pcm_decode_kernel (vapx_pcm_decode) uses;
//   - a 16 kHz class stores the decoded samples straight to the output with vector stores: no window, no barrier;
//   - any other rate: the samples land in LDS behind the stream's history [H], the new history is stored back, and every output is one
//     resample_dot chain over the tap tables resample_whole_kernel (vapx_resample) reads.  A stream has no future samples, so its 16 kHz
//     stream is the whole-signal Y delayed by d blocks (resample.hip): the first d blocks after a reset (`started` clear) are zero.
// One definition of each expansion and of the chain: a stream of class (f, r) in a table equals, bit for bit, the stream of a uniform
// engine of (f, r).  The tick moves about 40 MB at 4096 streams; nothing is tuned past coalesced access.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "input_classes.h"
#include "input_decode.h"

namespace {

// the row's dwords -> decoded samples in LDS (scalar LDS stores: the window starts H floats in, at no particular alignment)
template <int FMT>
__device__ __forceinline__ void decode_to_lds(const uint32_t* __restrict__ src, float* __restrict__ dst, int dwords, int tid) {
  for (int i = tid; i < dwords; i += 256) {
    const uint32_t w = src[i];
    if (FMT == VAPX_PCM_F32) {
      dst[i] = __uint_as_float(w);
    } else if (FMT == VAPX_PCM_S16) {
      dst[2 * i] = pcm_value((int)(short)(w & 0xFFFFu));
      dst[2 * i + 1] = pcm_value((int)(short)(w >> 16));
    } else {
      dst[4 * i] = pcm_code<FMT>(w & 0xFFu);
      dst[4 * i + 1] = pcm_code<FMT>((w >> 8) & 0xFFu);
      dst[4 * i + 2] = pcm_code<FMT>((w >> 16) & 0xFFu);
      dst[4 * i + 3] = pcm_code<FMT>(w >> 24);
    }
  }
}

// the row's dwords -> decoded samples in global memory (a 16 kHz class): one 4-, 8- or 16-byte store per lane.  dst is 16-byte aligned:
// the output buffer is, and a row (out_row: the hop, or L = hop + 320 for full frames) is a multiple of 16 samples
template <int FMT>
__device__ __forceinline__ void decode_to_out(const uint32_t* __restrict__ src, float* __restrict__ dst, int dwords, int tid) {
  for (int i = tid; i < dwords; i += 256) {
    const uint32_t w = src[i];
    if (FMT == VAPX_PCM_F32) {
      dst[i] = __uint_as_float(w);
    } else if (FMT == VAPX_PCM_S16) {
      float2 o;
      o.x = pcm_value((int)(short)(w & 0xFFFFu));
      o.y = pcm_value((int)(short)(w >> 16));
      *reinterpret_cast<float2*>(dst + 2 * i) = o;
    } else {
      float4 o;
      o.x = pcm_code<FMT>(w & 0xFFu);
      o.y = pcm_code<FMT>((w >> 8) & 0xFFu);
      o.z = pcm_code<FMT>((w >> 16) & 0xFFu);
      o.w = pcm_code<FMT>(w >> 24);
      *reinterpret_cast<float4*>(dst + 4 * i) = o;
    }
  }
}

// One workgroup per (batch slot, channel): LDS = taps | history [H] ++ this tick's hop_in decoded samples (classes off 16 kHz only).
__global__ __launch_bounds__(256) void input_classes_kernel(InputClassesArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, row = blockIdx.x, b = row >> 1, c = row & 1;
  const int pair = a.slots ? __builtin_amdgcn_readfirstlane(a.slots[b].cls) : 0;   // uniform over the workgroup: scalars
  const InputClassGeom g = a.cls[(pair >> (8 * c)) & 0xFF];                        // this channel's class
  const int n_in = g.orig ? g.hop_in : a.out_row;   // a 16 kHz row is as long as the row stepped
  const int row_bytes = n_in * pcm_bytes_per_sample(g.fmt), dwords = row_bytes >> 2;   // every row is a multiple of 16 samples
  size_t byte_off;
  if (a.slots) {   // channel 2's row follows channel 1's, which is of channel 1's class (a table's 16 kHz row is the hop: hop_in)
    const InputClassGeom g1 = a.cls[pair & 0xFF];
    byte_off = (size_t)a.slots[b].byte_off + (c ? (size_t)g1.hop_in * pcm_bytes_per_sample(g1.fmt) : 0);
  } else {
    byte_off = ((size_t)b * 2 + c) * row_bytes;   // no descriptors: a uniform engine, rows back to back
  }
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.in + byte_off);
  float* o = a.out + (long)row * a.out_row;

  if (g.orig == 0) {   // 16 kHz: decode straight to the output
    switch (g.fmt) {
      case VAPX_PCM_F32: decode_to_out<VAPX_PCM_F32>(src, o, dwords, tid); break;
      case VAPX_PCM_S16: decode_to_out<VAPX_PCM_S16>(src, o, dwords, tid); break;
      case VAPX_PCM_MULAW: decode_to_out<VAPX_PCM_MULAW>(src, o, dwords, tid); break;
      default: decode_to_out<VAPX_PCM_ALAW>(src, o, dwords, tid); break;
    }
    return;
  }

  float* th = lds;
  float* buf = lds + kTapSlots;
  const int sid = a.ids ? a.ids[b] : b;
  const float* tp = taps_of(g.orig);
  for (int i = tid; i < g.nnew * g.K; i += 256) th[i] = tp[i];
  float* hs = a.hist + (long)sid * a.rec + c * (a.slots ? a.rec >> 1 : g.H);   // a table: half the record, whatever the other channel's H
  for (int i = tid; i < g.H; i += 256) buf[i] = hs[i];
  switch (g.fmt) {
    case VAPX_PCM_F32: decode_to_lds<VAPX_PCM_F32>(src, buf + g.H, dwords, tid); break;
    case VAPX_PCM_S16: decode_to_lds<VAPX_PCM_S16>(src, buf + g.H, dwords, tid); break;
    case VAPX_PCM_MULAW: decode_to_lds<VAPX_PCM_MULAW>(src, buf + g.H, dwords, tid); break;
    default: decode_to_lds<VAPX_PCM_ALAW>(src, buf + g.H, dwords, tid); break;
  }
  const bool fresh = a.started[sid * 2 + c] == 0;   // no tick since the stream's reset: Y has no samples before its block 0
  __syncthreads();
  for (int i = tid; i < g.H; i += 256) hs[i] = buf[g.hop_in + i];   // hop_in >= 160 > H: the new history is all of this tick
  if (tid == 0) a.started[sid * 2 + c] = 1;
  for (int m = tid; m < a.out_row; m += 256) {   // out_row is the hop: full frames are a 16 kHz engine's
    const int j = m / g.nnew, p = m - j * g.nnew;
    const float v = resample_dot(th + p * g.K, buf + g.orig * j, g.K);   // last index read: hop_in + 2 width - 1 < H + hop_in
    o[m] = (fresh && j < g.d) ? 0.f : v;
  }
}

}  // namespace

size_t input_classes_lds_floats(const InputClassGeom* cls, int n_cls) {
  size_t win = 0;
  for (int i = 0; i < n_cls; ++i)
    if (cls[i].orig && (size_t)(cls[i].H + cls[i].hop_in) > win) win = (size_t)(cls[i].H + cls[i].hop_in);
  return win ? kTapSlots + win : 0;   // 48 + 40 + 9600 floats (about 39 KB) at 48 kHz and 5 Hz
}

hipError_t launch_input_classes(const InputClassesArgs& a, int n, size_t lds_floats, hipStream_t st) {
  hipLaunchKernelGGL(input_classes_kernel, dim3((unsigned)n * 2), dim3(256), lds_floats * sizeof(float), st, a);
  return hipGetLastError();
}
