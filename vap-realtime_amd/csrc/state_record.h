// A stream's state record (include/vapx.h "Bulk state export / import"), described once: where each section starts, what the eight header
// words are and which rule a header offered for import breaks first.  Plain C++17, no HIP: engine.hip (host) and state_io.hip (kernels)
// include it, and tests/native/state_record_check.cpp compiles this header alone and holds it against figures written out by hand.
#pragma once
#include <cstdint>

#include "../../include/vapx.h"

constexpr int kStateLstmFloats = 2 * 2 * 256;   // lstm [2 ch][2 (h, c)][256]
constexpr int kStateCarryFloats = 2 * 320;      // carry [2][320]

enum StateHeaderWord {   // the header: VAPX_STATE_HEADER_FLOATS int32 words, stored in the float slots bit for bit
  SH_MAGIC = 0, SH_CTX_FRAMES, SH_FRAME_HZ, SH_BITS, SH_N_FRAMES, SH_MODE, SH_INPUT_HZ, SH_STARTED, SH_WORDS
};
static_assert(SH_WORDS == VAPX_STATE_HEADER_FLOATS, "vapx.h and the header words disagree");

enum StateSection { SEC_RING = 1, SEC_LSTM = 2, SEC_CARRY = 4, SEC_HISTORY = 8, SEC_CACHE = 16 };   // StateIoArgs::sections

// float offsets of a record's sections, in the order they travel; -1: the record has no such section
struct StateLayout {
  long header, lstm, carry, history, ring, cache, total;
  int sections() const {   // every section the record has
    return SEC_RING | (lstm >= 0 ? SEC_LSTM : 0) | (carry >= 0 ? SEC_CARRY : 0) | (history >= 0 ? SEC_HISTORY : 0) | (cache >= 0 ? SEC_CACHE : 0);
  }
};

// with_state: LSTM + carry travel (a stand-alone engine or a trunk leader); rs_rec: floats of the resampler history, a multiple of 4 (0: none)
inline StateLayout state_layout(int T, bool with_state, int rs_rec, bool with_cache) {
  StateLayout l;
  long at = 0;
  const auto take = [&at](bool present, long floats) { const long o = present ? at : -1; if (present) at += floats; return o; };
  l.header = take(true, VAPX_STATE_HEADER_FLOATS);
  l.lstm = take(with_state, kStateLstmFloats);
  l.carry = take(with_state, kStateCarryFloats);
  l.history = take(rs_rec > 0, rs_rec);
  l.ring = take(true, (long)2 * T * 256);
  l.cache = take(with_cache, (long)2 * T * 768);
  l.total = at;
  return l;
}

// what an importing engine expects of a record's header: its window and rate, its input rate (0: none of its own, no resampler history),
// whether it is a trunk follower (no LSTM + carry), the call's VAPX_STATE_CACHE and whether the engine runs the split-precision path
struct StateExpect { int ctx_frames, frame_hz, input_hz; bool follower, with_cache, split; };

enum StateHeaderFault {   // in the order the rules are evaluated
  SHF_NONE = 0, SHF_MAGIC, SHF_CTX_FRAMES, SHF_FRAME_HZ, SHF_ROLE, SHF_INPUT_RATE, SHF_CACHE, SHF_CACHE_PATH, SHF_N_FRAMES
};

// the first rule the header breaks
inline StateHeaderFault state_header_check(const int32_t hd[SH_WORDS], const StateExpect& e) {
  const int bits = hd[SH_BITS];
  if (hd[SH_MAGIC] != VAPX_STATE_MAGIC) return SHF_MAGIC;
  if (hd[SH_CTX_FRAMES] != e.ctx_frames) return SHF_CTX_FRAMES;
  if (hd[SH_FRAME_HZ] != e.frame_hz) return SHF_FRAME_HZ;
  if (((bits & VAPX_STATE_HAS_LSTM) != 0) == e.follower) return SHF_ROLE;
  if (((bits & VAPX_STATE_HAS_RESAMPLE) != 0) != (e.input_hz != 0) || hd[SH_INPUT_HZ] != e.input_hz) return SHF_INPUT_RATE;
  if (((bits & VAPX_STATE_HAS_CACHE) != 0) != e.with_cache) return SHF_CACHE;
  if (e.with_cache && ((bits & VAPX_STATE_CACHE_SPLIT) != 0) != e.split) return SHF_CACHE_PATH;
  if (hd[SH_N_FRAMES] < 0 || hd[SH_N_FRAMES] > e.ctx_frames) return SHF_N_FRAMES;
  return SHF_NONE;
}
