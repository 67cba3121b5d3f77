// The engine's geometry and its batch-linear scratch buffers, described once.  Plain C++17, no HIP: tests/native/engine_buffers_check.cpp
// compiles this header alone and holds the table against the sizes written out by hand.
//
// Every buffer of Scratch is linear in the batch index: a sub-batch that starts at stream slot b0 is the same struct with every pointer
// advanced by b0 x (elements per slot).  kScratchTable has one row per buffer; vapx_create (allocation), Scratch::slice (offsets), the
// VAPX_POISON_SCRATCH refill, vapx_peek (name -> pointer, size), vapx_attach_trunk (what a follower releases) and vapx_destroy all walk it,
// so a buffer is added, resized or renamed in exactly one place.
#pragma once
#include <cstddef>
#include <cstring>

#include "../../include/vapx.h"

constexpr int kCarrySamples = 320;   // VAPX_PAD of common.h (engine.hip asserts it): samples of the previous frame in front of a hop

struct Geometry {
  int hop, L, P[5], ncpc, T;   // samples per frame, frame + carry, positions after conv0..4, CPC steps per frame, window rows
};

// the CPC encoder's strides (5, 4, 2, 2, 2) on one frame of `hz` frames per second; T is the caller's (ctx_frames)
inline Geometry geometry(int hz, int T = 0) {
  Geometry g;
  g.hop = 16000 / hz;
  g.L = g.hop + kCarrySamples;
  g.P[0] = g.L / 5;
  g.P[1] = g.P[0] / 4;
  g.P[2] = g.P[1] / 2;
  g.P[3] = g.P[2] / 2;
  g.P[4] = g.P[3] / 2;
  g.ncpc = g.P[4] - 2;
  g.T = T;
  return g;
}

// vapx_prefill: frames of n streams that one pass through the step's scratch holds.  Every encoder buffer is sized for max_batch entries and
// a (stream, frame) pair is an entry, so floor(max_batch / n) frames fit; n > max_batch / 2 leaves one frame per pass
// (engine.prefill_chunks in ../engine.py restates the plan for the host-side tests)
inline int prefill_chunk_frames(int max_batch, int n) {
  const int fc = n > 0 ? max_batch / n : 0;
  return fc < 1 ? 1 : fc;
}

struct Scratch {
  float* out_dev = nullptr;   // [B][VAPX_OUT_STRIDE] the step's output rows before they leave (or the caller's device block instead)
  int *bn = nullptr, *bhead = nullptr, *rot = nullptr;
  float *h0 = nullptr, *h1 = nullptr, *h2 = nullptr, *h3 = nullptr, *z = nullptr, *gx = nullptr, *lstm_out = nullptr, *e = nullptr;
  float* xl[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // layer inputs/outputs: x0, o, stereo0..2
  float *xn = nullptr, *xmid = nullptr, *att = nullptr, *qkv = nullptr, *qx = nullptr, *kvx = nullptr;
  float* last[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [B*2][256] each: x, xn, q, att, xmid, out (last-row path)
  float *en = nullptr, *qkv_new = nullptr;   // [B*2][256], [B*2][768]: LN0(e) and layer-0 Q|K|V of the new row
  float* lffn = nullptr;                     // [B*2][768] FFN hidden of the last-row path
  inline Scratch slice(size_t b0, const Geometry& g) const;
};

struct ScratchSlot { float** f; int** i; };   // a Scratch member: exactly one of the two is set

struct ScratchRow {
  const char* member;                       // the Scratch member, as written in the code
  ScratchSlot (*slot)(Scratch&);
  size_t (*per_slot)(const Geometry&);      // floats / ints per batch slot
  bool poison;                              // VAPX_POISON_SCRATCH refills it before every step (never: h0..h3, whose guard rows must stay
                                            // zero, and bn / bhead / rot, which conv0 or the window kernels write before anyone reads)
  bool encoder;                             // encoder scratch: a trunk follower releases it (vapx_attach_trunk)
  const char* peek;                         // vapx_peek name, or null
};

#define VAPX_F(m) #m, [](Scratch& s) { return ScratchSlot{&s.m, nullptr}; }
#define VAPX_I(m) #m, [](Scratch& s) { return ScratchSlot{nullptr, &s.m}; }
#define VAPX_N(expr) [](const Geometry& g) { (void)g; return (size_t)(expr); }
inline constexpr ScratchRow kScratchTable[] = {
    //  member            per batch slot                      poison encoder peek
    {VAPX_F(out_dev),  VAPX_N(VAPX_OUT_STRIDE),               true,  false, nullptr},
    {VAPX_I(bn),       VAPX_N(1),                             false, false, nullptr},
    {VAPX_I(bhead),    VAPX_N(1),                             false, false, nullptr},
    {VAPX_I(rot),      VAPX_N(1),                             false, false, nullptr},
    {VAPX_F(h0),       VAPX_N(2 * (g.P[0] + 4) * 256),        false, true,  "h0"},   // conv outputs with their zero guard rows
    {VAPX_F(h1),       VAPX_N(2 * (g.P[1] + 2) * 256),        false, true,  "h1"},
    {VAPX_F(h2),       VAPX_N(2 * (g.P[2] + 2) * 256),        false, true,  "h2"},
    {VAPX_F(h3),       VAPX_N(2 * (g.P[3] + 2) * 256),        false, true,  "h3"},
    {VAPX_F(z),        VAPX_N(2 * g.ncpc * 256),              true,  true,  "z"},
    {VAPX_F(lstm_out), VAPX_N(2 * g.ncpc * 256),              true,  true,  "lstm_out"},
    {VAPX_F(gx),       VAPX_N(2 * g.ncpc * 1024),             true,  true,  nullptr},
    {VAPX_F(e),        VAPX_N(2 * 256),                       true,  false, "e"},
    {VAPX_F(xl[0]),    VAPX_N((size_t)2 * g.T * 256),         true,  false, "x0"},
    {VAPX_F(xl[1]),    VAPX_N((size_t)2 * g.T * 256),         true,  false, "o"},
    {VAPX_F(xl[2]),    VAPX_N((size_t)2 * g.T * 256),         true,  false, "stereo0"},
    {VAPX_F(xl[3]),    VAPX_N((size_t)2 * g.T * 256),         true,  false, "stereo1"},
    {VAPX_F(xl[4]),    VAPX_N((size_t)2 * g.T * 256),         true,  false, "stereo2"},
    {VAPX_F(xn),       VAPX_N((size_t)2 * g.T * 256),         true,  false, nullptr},
    {VAPX_F(xmid),     VAPX_N((size_t)2 * g.T * 256),         true,  false, "comb"},   // nod mode: [B][T][256] of it (vapx_peek)
    {VAPX_F(att),      VAPX_N((size_t)2 * g.T * 256),         true,  false, nullptr},
    {VAPX_F(qkv),      VAPX_N((size_t)2 * g.T * 768),         true,  false, nullptr},
    {VAPX_F(qx),       VAPX_N((size_t)2 * g.T * 256),         true,  false, nullptr},
    {VAPX_F(kvx),      VAPX_N((size_t)2 * g.T * 512),         true,  false, nullptr},
    {VAPX_F(last[0]),  VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(last[1]),  VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(last[2]),  VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(last[3]),  VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(last[4]),  VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(last[5]),  VAPX_N(2 * 256),                       true,  false, "last"},
    {VAPX_F(en),       VAPX_N(2 * 256),                       true,  false, nullptr},
    {VAPX_F(qkv_new),  VAPX_N(2 * 768),                       true,  false, nullptr},
    {VAPX_F(lffn),     VAPX_N(2 * 768),                       true,  false, nullptr},
};
#undef VAPX_F
#undef VAPX_I
#undef VAPX_N

inline Scratch Scratch::slice(size_t b0, const Geometry& g) const {
  Scratch s = *this;
  for (const ScratchRow& r : kScratchTable) {
    const ScratchSlot p = r.slot(s);
    const size_t off = b0 * r.per_slot(g);
    if (p.f) { if (*p.f) *p.f += off; }   // a released buffer stays null
    else if (*p.i) *p.i += off;
  }
  return s;
}

inline void* scratch_ptr(const ScratchRow& r, Scratch& s) {
  const ScratchSlot p = r.slot(s);
  return p.f ? (void*)*p.f : (void*)*p.i;
}

inline const ScratchRow* scratch_row_by_peek(const char* name) {
  for (const ScratchRow& r : kScratchTable)
    if (r.peek && !strcmp(r.peek, name)) return &r;
  return nullptr;
}

// Two decisions an engine makes once, at vapx_create, from its flags, mode and window.
// Layer 0 reads the rings in place (no chronological copy, so no x0): always for the fused short-window block, and for long windows when
// they run the fused long-window chain (the GEMM-chain variants need x0 as a plain buffer)
inline bool ring_direct_for(int flags, int T) {
  return !(flags & VAPX_FLAG_MATERIALIZE_X0) && (T <= 64 || !(flags & VAPX_FLAG_UNFUSED_PROJ));
}
// The last layer runs on the newest row alone (the nod variant emits p_bc for every row of the window, which needs the whole last layer)
inline bool prune_last_for(int flags, int mode) { return !(flags & VAPX_FLAG_FULL_LAST_LAYER) && mode != VAPX_MODE_NOD; }

// The latest pass through the scratch buffers, as vapx_peek and vapx_join find it.  Who writes what:
//   vapx_step, leader      entries = n, groups, prefill = false; tail_fused = false, then true if a group's encoder ran conv_tail_kernel
//   vapx_step, follower    entries = n, groups, prefill = false (tail_fused stays: it has no encoder)
//   vapx_prefill           per chunk: entries = (frame, stream) pairs, frame-major, groups = 1, prefill = true, tail_fused as a leader step
//   vapx_encode_audio      entries = n, prefill = false, tail_fused as a leader step (groups stays)
//   vapx_transformer_maps  entries = n, prefill = false (groups and tail_fused stay)
struct PassRecord {
  int entries = 0, groups = 1;
  bool prefill = false;      // no lstm_out (the prefill's LSTM launch keeps it to itself) and no transformer buffer
  bool tail_fused = false;   // h2 / h3 were not written
};

// vapx_peek's refusals: each is a printf format of the arguments (name, name), but kPeekCombSplit, which takes the number of groups
inline constexpr char kPeekNotInPrefill[] =
    "\"%s\" is not written by vapx_prefill (its LSTM launch keeps lstm_out to itself and no transformer layer runs): "
    "after a prefill only h0 .. h3, z and e of its last chunk exist; step to peek \"%s\"";
inline constexpr char kPeekInLds[] = "\"%s\" stays in LDS in the fused conv tail; create the engine with VAPX_FLAG_UNFUSED_CONV to peek it";
inline constexpr char kPeekX0InRing[] = "\"x0\" is read straight from the ring; create the engine with VAPX_FLAG_MATERIALIZE_X0 to peek it";
inline constexpr char kPeekStereo2Pruned[] =
    "\"stereo2\" is only materialised with VAPX_FLAG_FULL_LAST_LAYER (default: last layer runs on the newest row only)";
inline constexpr char kPeekLastEveryRow[] =
    "\"last\" exists only where the last layer runs on the newest row alone; this engine (VAPX_FLAG_FULL_LAST_LAYER "
    "or nod mode) computes every row: peek \"stereo2\" and take row n - 1";
inline constexpr char kPeekCombNotNod[] =
    "\"comb\" is only materialised in nod mode (vap / bc: the combinator of the newest row stays inside head_kernel)";
inline constexpr char kPeekCombSplit[] =
    "\"comb\" is not contiguous when the latest step ran in %d overlap groups; step with groups = 1 to peek it";
inline constexpr char kPeekUnknown[] = "unknown buffer '%s'";
inline constexpr char kPeekReleased[] = "\"%s\" is released: this engine is a trunk follower, peek its leader";

// What exists after the latest pass depends on the path it took: null, or why buffer `name` cannot be read (one of the formats above).
// `released`: the engine has freed the buffer of that name (vapx_attach_trunk, a follower's encoder scratch)
inline const char* peek_refusal(const PassRecord& pass, int mode, bool ring_direct, bool prune_last, bool released, const char* name) {
  const auto is = [name](const char* s) { return !strcmp(name, s); };
  if (pass.prefill && !(is("h0") || is("h1") || is("h2") || is("h3") || is("z") || is("e"))) return kPeekNotInPrefill;
  if ((is("h2") || is("h3")) && pass.tail_fused) return kPeekInLds;   // what the encoder ran, not a guess from the batch: the fused tail's
                                                                      // 512-stream limit holds per overlap group
  if (is("x0") && ring_direct) return kPeekX0InRing;
  if (is("stereo2") && prune_last) return kPeekStereo2Pruned;
  if (is("last") && !prune_last) return kPeekLastEveryRow;   // the newest row of every (stream, channel): fused block and ten-launch path alike
  if (is("comb") && mode != VAPX_MODE_NOD) return kPeekCombNotNod;
  if (is("comb") && pass.groups > 1) return kPeekCombSplit;   // a group's block starts at its first row of the [B*2*T]-row scratch, twice
                                                              // the stride of the [nb*T] rows it holds
  if (!scratch_row_by_peek(name)) return kPeekUnknown;
  return released ? kPeekReleased : nullptr;
}
