// Input at 8 / 32 / 48 kHz -> the model's 16 kHz on the device (vapx_set_input_rate, vapx_resample; include/vapx.h "Input rate").
// The filter is torchaudio.functional.resample's default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), restated in
// vap-realtime_amd/resample.py, which also writes the fp32 tap tables of resample_taps.h.  With orig = in_hz / g, new = 16000 / g:
//   Y[new*i + p] = sum_k h[p][k] * x[orig*i + k - width],  k = 0 .. K-1,  x = 0 outside the signal
// vapx_resample turns whole signals into Y.  An engine's stream has no future samples: its 16 kHz stream is Y delayed by
// d = ceil(width / orig) = 7 blocks (0.875 ms at 8 kHz, 0.4375 ms at 32 and 48 kHz), z[m] = Y[m - new*d] and zero for m < new*d; a tick
// needs the last H = orig*d + width input samples of the stream's earlier ticks.  That streaming form is input_classes_kernel
// (input_classes.hip), the engine's one input launch; this file keeps the geometry both share and the whole-signal kernel.
// Both stage their input window in LDS with coalesced 4-byte loads (lane i at base + 4 i), keep the taps in LDS (copied from constant
// memory) and produce every output with resample_dot: one fmaf chain over k = 0 .. K-1.  The streaming launch and the whole-signal
// kernel therefore agree bit for bit.
#include <hip/hip_runtime.h>

#include "input_decode.h"   // the tap tables, taps_of and resample_dot: shared with input_classes.hip
#include "vap_kernels.h"

namespace {

// Whole signals: a workgroup makes 256 output blocks (256 * new outputs) of one row from a window of orig * 255 + K inputs.
constexpr int kWholeBlocks = 256;
constexpr int kWholeWindow = 3 * (kWholeBlocks - 1) + 41;   // the largest: 48 kHz
__global__ __launch_bounds__(256) void resample_whole_kernel(const float* __restrict__ x, float* __restrict__ y, long n_in, long n_out,
                                                             int orig, int nnew, int width, int K, long row0) {
  __shared__ float th[kTapSlots];
  __shared__ float win[kWholeWindow];
  const int tid = threadIdx.x;
  const long r = row0 + blockIdx.y, i0 = (long)blockIdx.x * kWholeBlocks;
  const float* tp = taps_of(orig);
  for (int i = tid; i < nnew * K; i += 256) th[i] = tp[i];
  const float* xr = x + r * n_in;
  const long s0 = orig * i0 - width;
  const int wlen = orig * (kWholeBlocks - 1) + K;
  for (int i = tid; i < wlen; i += 256) {
    const long s = s0 + i;
    win[i] = (s >= 0 && s < n_in) ? xr[s] : 0.f;
  }
  __syncthreads();
  for (int q = tid; q < kWholeBlocks * nnew; q += 256) {
    const int j = q / nnew, p = q - j * nnew;
    const long m = nnew * i0 + q;
    if (m < n_out) y[r * n_out + m] = resample_dot(th + p * K, win + orig * j, K);
  }
}

}  // namespace

bool resample_geometry(int in_hz, ResampleGeom* g) {
  switch (in_hz) {
    case 8000: *g = {1, 2, 7, 15, 7, 14}; return true;
    case 32000: *g = {2, 1, 13, 28, 7, 27}; return true;
    case 48000: *g = {3, 1, 19, 41, 7, 40}; return true;
  }
  return false;
}

hipError_t launch_resample_whole(const ResampleGeom& g, long rows, long n_in, const float* x, float* y, hipStream_t st) {
  const long n_out = (g.nnew * n_in + g.orig - 1) / g.orig;
  const long per = (long)kWholeBlocks * g.nnew;
  const unsigned gx = (unsigned)((n_out + per - 1) / per);
  for (long r0 = 0; r0 < rows; r0 += 32768) {   // gridDim.y is a 16-bit quantity
    const unsigned gy = (unsigned)(rows - r0 < 32768 ? rows - r0 : 32768);
    hipLaunchKernelGGL(resample_whole_kernel, dim3(gx, gy), dim3(256), 0, st, x, y, n_in, n_out, g.orig, g.nnew, g.width, g.K, r0);
  }
  return hipGetLastError();
}
