// Input in the sample format it already has: 16-bit linear PCM and G.711 mu-law / A-law -> the fp32 the model computes in, on the device
// (include/vapx.h "Input format").  This file is vapx_pcm_decode, a block of samples of any length; an engine with an input format
// (vapx_set_input_format) decodes its ticks in input_classes_kernel (input_classes.hip), with the same device functions of input_decode.h.  The definition is vap-realtime_amd/pcm.py, which also writes
// the two 256-entry tables of pcm_tables.h:  s16: float(v) * 2^-15;  mulaw / alaw: float(table[c]) * 2^-15.  Every value is exact in
// fp32 and integer zero converts to +0.0f, so a stream stepped in a raw format equals, bit for bit, one fed the decoded floats.
//
// G.711 is expanded by the CLOSED FORM in integer ALU (a handful of shifts and adds per code), not by a table in LDS: no LDS, no barrier,
// no constant-memory traffic.  input_decode.h holds the closed forms to pcm_tables.h for all 256 codes at compile time; the host
// side (the front-end's echo, csrc/ingest.cpp) reads the tables.
//
// The block is flat: n samples in a row.  Lane i reads the aligned dword at base + 4 i (two s16 samples or four codes) and writes its
// outputs with one 8-byte or one 16-byte store; the kernel is bound by that traffic and nothing is tuned past the access pattern.  A
// sample count that does not fill the last dword is finished by that dword's lane with single loads and stores, so nothing is read or
// written past n samples.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vapx.h"
#include "input_decode.h"   // the closed forms, pcm_value and pcm_code: shared with input_classes.hip
#include "vap_kernels.h"

namespace {

// n samples at src (dword-aligned) -> n floats at dst (8-byte aligned for s16, 16-byte aligned for G.711)
template <int FMT>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const uint32_t* __restrict__ src, float* __restrict__ dst, long n) {
  constexpr int PER = FMT == VAPX_PCM_S16 ? 2 : 4;   // samples in a dword
  const long full = n / PER;                         // whole dwords
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < full; i += stride) {
    const uint32_t w = src[i];
    if (FMT == VAPX_PCM_S16) {
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
  if (blockIdx.x == 0 && threadIdx.x == 0) {         // the samples of a last, partial dword
    for (long s = full * PER; s < n; ++s) {
      if (FMT == VAPX_PCM_S16) dst[s] = pcm_value((int)reinterpret_cast<const short*>(src)[s]);
      else dst[s] = pcm_code<FMT>(reinterpret_cast<const uint8_t*>(src)[s]);
    }
  }
}

}  // namespace

hipError_t launch_pcm_decode(int format, long n, const void* src, float* dst, hipStream_t st) {
  const int per = format == VAPX_PCM_S16 ? 2 : 4;
  const long dwords = (n + per - 1) / per;
  long blocks = (dwords + 255) / 256;
  if (blocks > 16384) blocks = 16384;                // the loop strides over the rest
  const dim3 grid((unsigned)blocks), wg(256);
  const uint32_t* s = (const uint32_t*)src;
  switch (format) {
    case VAPX_PCM_S16: hipLaunchKernelGGL(pcm_decode_kernel<VAPX_PCM_S16>, grid, wg, 0, st, s, dst, n); break;
    case VAPX_PCM_MULAW: hipLaunchKernelGGL(pcm_decode_kernel<VAPX_PCM_MULAW>, grid, wg, 0, st, s, dst, n); break;
    case VAPX_PCM_ALAW: hipLaunchKernelGGL(pcm_decode_kernel<VAPX_PCM_ALAW>, grid, wg, 0, st, s, dst, n); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
