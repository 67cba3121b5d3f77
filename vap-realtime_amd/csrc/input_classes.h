// The engine's input launch (vapx_set_input_rate / _format / _classes; include/vapx.h "Input rate", "Input format", "Input classes"):
// what engine.hip hands to input_classes.hip.  Plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vapx.h"

// one class as the kernel reads it: the resampler's geometry (orig = 0: the class is 16 kHz, no window), samples per channel and tick, format
struct InputClassGeom { int orig, nnew, width, K, d, H, hop_in, fmt; };

// one batch slot of a tick: where channel 1's row starts in the packed block (channel 2's follows it), and the two channels' classes
struct InputSlot { uint32_t byte_off; int32_t cls; };   // cls: input_slot_classes(c1, c2)
inline int32_t input_slot_classes(int c1, int c2) { return c1 | (c2 << 8); }   // VAPX_MAX_INPUT_CLASSES = 16 fits a byte

struct InputClassesArgs {
  const unsigned char* in;   // the block: packed slots, 16-byte aligned (a table), or [n][2][row] samples of class 0, dword-aligned (slots == null)
  const InputSlot* slots;    // [n], or null: a uniform engine, slot b is class 0 at b * (bytes of its two rows)
  const int* ids;            // [n] stream ids (device) or null = identity
  float* hist;               // [S][rec]: a stream's input samples of its earlier ticks.  slots == null: [2][H], then padding (what a state
                             // record carries).  A table: channel c's H(its class) floats at c * rec / 2, whatever the other channel's class
  int* started;              // [S][2]: the (stream, channel) has consumed a tick since its reset
  float* out;                // [n][2][out_row] the 16 kHz samples conv0 takes
  int rec;
  int out_row;               // samples of an output row, and of a 16 kHz class's input row: the hop; a uniform 16 kHz engine stepped with
                             // full frames: L (the caller's carry in front).  A multiple of 16
  InputClassGeom cls[VAPX_MAX_INPUT_CLASSES];
};

// lds_floats: the dynamic LDS of the engine's largest class (input_classes_lds_floats over the table)
size_t input_classes_lds_floats(const InputClassGeom* cls, int n_cls);
hipError_t launch_input_classes(const InputClassesArgs& a, int n, size_t lds_floats, hipStream_t st);
