// The device functions every input kernel shares: the G.711 / s16 expansions of pcm.hip and the resampler's tap tables and fmaf chain of
// resample.hip.  pcm_decode_kernel, resample_whole_kernel and input_classes_kernel (input_classes.hip, the engine's one input launch) all
// include this header, so there is ONE definition of each expansion and ONE of the chain: a stream stepped through any of them sees the
// same bits.
// The definitions are vap-realtime_amd/pcm.py (tables of pcm_tables.h) and vap-realtime_amd/resample.py (taps of resample_taps.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vapx.h"
#include "pcm_tables.h"
#include "resample_taps.h"

namespace {

// ---- sample formats -----------------------------------------------------------------------------------------------------------------
// bytes of one sample, on the host and in the kernels; 0: unknown format id
__host__ __device__ constexpr int pcm_bytes_per_sample(int format) {
  return format == VAPX_PCM_F32 ? 4 : format == VAPX_PCM_S16 ? 2 : (format == VAPX_PCM_MULAW || format == VAPX_PCM_ALAW) ? 1 : 0;
}

// G.711 is expanded by the CLOSED FORM in integer ALU (a handful of shifts and adds per code), not by a table in LDS: no LDS, no barrier,
// no constant-memory traffic.  The static_assert below holds the closed forms to pcm_tables.h for all 256 codes at compile time.
__host__ __device__ constexpr int mulaw_linear(unsigned c) {
  c = ~c & 0xFFu;
  const int e = (int)(c >> 4) & 7, m = (int)(c & 15u);
  const int t = (((m << 3) + 0x84) << e) - 0x84;
  return (c & 0x80u) ? -t : t;
}

__host__ __device__ constexpr int alaw_linear(unsigned c) {
  c = (c ^ 0x55u) & 0xFFu;
  const int e = (int)(c >> 4) & 7, m = (int)(c & 15u);
  const int t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
  return (c & 0x80u) ? t : -t;
}

constexpr short kMulawTable[256] = {VAPX_PCM_MULAW_TABLE};
constexpr short kAlawTable[256] = {VAPX_PCM_ALAW_TABLE};
constexpr bool closed_forms_match_tables() {
  for (unsigned c = 0; c < 256; ++c)
    if (mulaw_linear(c) != kMulawTable[c] || alaw_linear(c) != kAlawTable[c]) return false;
  return true;
}
static_assert(closed_forms_match_tables(), "the closed forms of input_decode.h and pcm_tables.h (vap-realtime_amd/pcm.py) disagree");

// one sample: 16-bit linear -> fp32.  Exact; (float)0 is +0.0f
__device__ __forceinline__ float pcm_value(int v) { return (float)v * 0x1p-15f; }

template <int FMT>
__device__ __forceinline__ float pcm_code(unsigned c) {
  return pcm_value(FMT == VAPX_PCM_MULAW ? mulaw_linear(c) : alaw_linear(c));
}

// ---- resampler ----------------------------------------------------------------------------------------------------------------------
constexpr int kTapSlots = 48;   // floats reserved for h[new][K]: 2 x 15, 1 x 28, 1 x 41

__constant__ float c_taps_8k[] = {VAPX_RESAMPLE_TAPS_8000};
__constant__ float c_taps_32k[] = {VAPX_RESAMPLE_TAPS_32000};
__constant__ float c_taps_48k[] = {VAPX_RESAMPLE_TAPS_48000};
static_assert(sizeof(c_taps_8k) == 2 * 15 * 4 && sizeof(c_taps_32k) == 28 * 4 && sizeof(c_taps_48k) == 41 * 4, "tap tables");

__device__ __forceinline__ const float* taps_of(int orig) { return orig == 1 ? c_taps_8k : orig == 2 ? c_taps_32k : c_taps_48k; }

// one output: h = the phase's K taps, w = the K input samples under them.  The order of the chain is the definition.
__device__ __forceinline__ float resample_dot(const float* __restrict__ h, const float* __restrict__ w, int K) {
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(h[k], w[k], acc);
  return acc;
}

}  // namespace
