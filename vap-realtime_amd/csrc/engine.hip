// libvapx engine: owns device weights, per-stream state and scratch; orchestrates one VAP frame for
// a batch of streams (the C ABI of include/vapx.h).  Compiled with hipcc for gfx950 only.
//
// Reference path being replaced: VAPRealTime.__init__/process_vap, rvap/vap_main/vap_main.py:192-335.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/vapx.h"
#include "engine_buffers.h"
#include "fused_blocks.h"
#include "gemm_f32.h"
#include "input_classes.h"
#include "input_decode.h"   // pcm_bytes_per_sample
#include "vap_kernels.h"
#include "vapx_layout.h"

static_assert(kCarrySamples == VAPX_PAD, "engine_buffers.h and common.h disagree on the carry");

namespace {

thread_local std::string g_create_error;

struct Layer {
  const float *ln_self_g, *ln_self_b, *wqkv, *wproj;
  const float *ln_src_g, *ln_src_b, *wq_x, *wkv_x, *wproj_x;
  const float *ln_ffn_g, *ln_ffn_b, *w0, *w3;
  const float *w0f, *w3f, *wqkvf, *wkvxf, *wprojf, *wqxf, *wprojxf;   // fragment-major copies (fused blocks)
  const float *w0h, *w3h, *wqkvh, *wkvxh, *wprojh, *wqxh, *wprojxh;                             // split-precision (f16 hi/lo) fragment copies
  const float *wproj8, *wqx8, *wprojx8;   // the attention projections in the 8-wave format of the 64-row flat-row blocks (long windows)
  const float* wqkvp;                     // per-head Q|K|V weight stream of attention_proj_f16x3_kernel (layers >= 1)
  float hid_scale = 1.0f;   // split-precision path: static power-of-two scale of the GELU hidden row (1 unless the weights allow |gelu(h)| >= 2^15)
};

// everything outside the transformer layers, resolved once in vapx_create like layer[]: every member is required (vapx_create refuses a
// layout without it), except the copies a conv does not have (conv0: w16, wf; conv1: wf), which stay null and are never read
struct ConvW { const float *w, *w16, *wf, *b, *g, *beta; };   // conv i with its ChannelNorm; w16: split-precision GEMM copy, wf: conv_tail_kernel's
struct Weights {
  ConvW conv[5];
  const float *lstm_wih, *lstm_wih16, *lstm_whh, *lstm_b;
  const float *down_w, *down_wf, *down_b, *down_g, *down_beta;
  const float *l0_wqkv16, *l3_last16;
  const float *comb_wa, *comb_wb, *comb_waT, *comb_wbT, *comb_g, *comb_b;
  const float *head_w, *head_wT, *head_b, *vad_w, *vad_b, *aux_w, *aux_b;
};

// debug knob (env VAPX_GUARD_ZONES): every device allocation of the engine gets a 4 KiB canary zone on both sides; vapx_peek("guard_violations")
// counts the canary bytes that changed, i.e. out-of-bounds writes just past (or before) a buffer
constexpr size_t kGuardBytes = 4096;
bool guard_enabled() { static const bool on = getenv("VAPX_GUARD_ZONES") != nullptr; return on; }
struct GuardRec { char* base; size_t bytes; };
std::mutex g_guard_mu;
std::vector<GuardRec> g_guards;

template <typename T>
hipError_t dalloc(T** p, size_t n, bool zero = true) {
  const size_t bytes = n * sizeof(T);
  if (!guard_enabled()) {
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return e;
    return zero ? hipMemset(*p, 0, bytes) : hipSuccess;
  }
  char* base = nullptr;
  hipError_t e = hipMalloc((void**)&base, bytes + 2 * kGuardBytes);
  if (e != hipSuccess) return e;
  if ((e = hipMemset(base, 0xA5, kGuardBytes)) != hipSuccess) return e;
  if ((e = hipMemset(base + kGuardBytes + bytes, 0xA5, kGuardBytes)) != hipSuccess) return e;
  if (zero && bytes && (e = hipMemset(base + kGuardBytes, 0, bytes)) != hipSuccess) return e;
  *p = (T*)(base + kGuardBytes);
  std::lock_guard<std::mutex> lk(g_guard_mu);
  g_guards.push_back({base, bytes});
  return hipSuccess;
}
void dfree(void* p) {
  if (!p) return;
  if (guard_enabled()) {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    for (size_t i = 0; i < g_guards.size(); ++i)
      if (g_guards[i].base + kGuardBytes == (char*)p) {
        (void)hipFree(g_guards[i].base);
        g_guards.erase(g_guards.begin() + (long)i);
        return;
      }
  }
  (void)hipFree(p);
}
// canary bytes overwritten around ANY live allocation of the process's engines (device must be idle)
long guard_violations() {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  std::vector<unsigned char> host(kGuardBytes);
  long bad = 0;
  for (const GuardRec& r : g_guards)
    for (int side = 0; side < 2; ++side) {
      if (hipMemcpy(host.data(), side ? r.base + kGuardBytes + r.bytes : r.base, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      for (unsigned char c : host) bad += c != 0xA5;
    }
  return bad;
}

// true when p is page-locked host memory known to HIP (hipHostMalloc / hipHostRegister), i.e. a real async copy source / target
bool is_pinned_host(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

// A device block and the page-locked host block that pageable memory travels through, either way.  The pinned block is behind an event:
// the next upload reuses it only after the copy out of it has completed
template <typename T>
struct Staged {
  T *dev = nullptr, *pin = nullptr;
  size_t cap = 0, pin_cap = 0;   // elements the two blocks hold
  hipEvent_t evt = nullptr;      // the latest copy out of `pin` has completed
  // reserve: at least n elements in the device block (new ones zero-filled) and, on request, in the pinned one.  Contents are not kept, so
  // only while no copy is in flight; on failure the old blocks stay as they were
  hipError_t reserve_pinned(size_t n) {
    if (!evt) {
      hipError_t e = hipEventCreateWithFlags(&evt, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(evt, nullptr);
      if (e != hipSuccess) return e;
    }
    if (n <= pin_cap) return hipSuccess;
    T* np = nullptr;
    const hipError_t e = hipHostMalloc((void**)&np, n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return e;
    if (pin) (void)hipHostFree(pin);
    pin = np; pin_cap = n;
    return hipSuccess;
  }
  hipError_t reserve(size_t n, bool with_pinned) {
    T* nd = nullptr;
    hipError_t e = n > cap ? dalloc(&nd, n) : hipSuccess;
    if (e == hipSuccess && with_pinned) e = reserve_pinned(n);
    if (e != hipSuccess) { dfree(nd); return e; }
    if (nd) { dfree(dev); dev = nd; cap = n; }
    return hipSuccess;
  }
  // `pin`, for a caller that assembles its block there and then calls upload(pin, n, st): idle once the latest copy out of it is done
  hipError_t acquire_pinned() { return hipEventSynchronize(evt); }
  // host -> device: straight from a page-locked source (`direct`), else through `pin` (src == pin: assembled in place)
  hipError_t upload(const T* src, size_t n, hipStream_t st, bool direct = false) {
    if (direct) return hipMemcpyAsync(dev, src, n * sizeof(T), hipMemcpyHostToDevice, st);
    hipError_t e = src == pin ? hipSuccess : hipEventSynchronize(evt);
    if (e != hipSuccess) return e;
    if (src != pin) memcpy(pin, src, n * sizeof(T));
    if ((e = hipMemcpyAsync(dev, pin, n * sizeof(T), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    return hipEventRecord(evt, st);
  }
  // device (`src`, or this block) -> host: straight into the caller's block when it is page-locked (the copy is then still in flight on
  // return), else through `pin`, synchronised and copied on
  hipError_t download(void* dst, size_t bytes, hipStream_t st, const T* src = nullptr) {
    if (!src) src = dev;
    if (is_pinned_host(dst)) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    hipError_t e = hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) memcpy(dst, pin, bytes);
    return e;
  }
  void release() {
    dfree(dev);
    if (pin) (void)hipHostFree(pin);
    if (evt) (void)hipEventDestroy(evt);
    *this = Staged();
  }
};

}  // namespace

// per-stream state bases; for identity stream ids of a sub-batch starting at slot b0 the bases are
// simply advanced by b0 streams
struct StateView {
  float *ring, *ring_qkv, *h_state, *c_state, *carry;
  int* frames_seen;
};

struct vapx_engine : Geometry {
  vapx_config cfg;
  std::string err;

  float* w = nullptr;  // weight blob
  const vapx_layout::Entry* lay = nullptr;
  size_t lay_n = 0;
  Layer layer[4];
  Weights wt = {};

  // per-stream state
  float *ring = nullptr, *ring_qkv = nullptr, *h_state = nullptr, *c_state = nullptr, *carry = nullptr;
  int* frames_seen = nullptr;

  // scratch (max_batch); every buffer is linear in the batch index, so a sub-batch starting at
  // stream slot b0 is just the same struct with offset pointers (Scratch::slice, engine_buffers.h)
  Scratch sc;
  Staged<float> audio;   // host audio: device block of the step, [max_batch][2][L] floats, more where an input class's largest slot needs it;
                         // pageable memory is staged through the pinned one (vapx_host_alloc memory skips it)
  Staged<int> ids;       // host stream ids of a step
  Staged<float> out;     // pinned block only: a step's output rows (sc.out_dev) on their way to pageable memory
  bool ring_direct = false, prune_last = false;   // decided once, in vapx_create (engine_buffers.h)
  PassRecord pass;       // the latest pass through the scratch buffers
  // intra-tick overlap: the batch is split into groups that run on their own HIP streams
  static constexpr int kMaxGroups = 8;
  hipStream_t gstream[kMaxGroups] = {};
  hipEvent_t gdone[kMaxGroups] = {};
  hipEvent_t gstart = nullptr;
  int n_groups = 1;
  // debug knob (env VAPX_POISON_SCRATCH): every scratch buffer the table marks is refilled with NaN bit patterns before each step and the
  // rings start as NaNs, so a kernel that consumes anything it (or an earlier kernel of the same tick) did not write shows up as a non-finite output
  bool poison = false;
  // debug knob (env VAPX_FORCE_ATTENTION_XL, read once per engine in vapx_create): every long window of the fp32 path runs
  // attention_xl_kernel, so tests can hold it against attention_long2_kernel on windows both kernels take
  bool force_xl = false;
#ifdef VAPX_TRACE   // debug build only (make trace -> libvapx_trace.so): per-workgroup phase stamps, tools/ffn_trace.py / tools/attn_trace.py
  unsigned long long* ffn_trace = nullptr;   // env VAPX_FFN_TRACE=<file>: phase stamps of the layer-0 FFN block's workgroups
  unsigned long long* attn_trace = nullptr;  // env VAPX_ATTN_TRACE=<file>: phase stamps of the layer-1 self-attention block's workgroups
  size_t ffn_trace_wgs = 0, attn_trace_wgs = 0;
  std::string ffn_trace_path, attn_trace_path;
#endif
  // the engine's input (input_classes.hip): n_cls = 0, the caller's audio is 16 kHz fp32 and goes to conv0 as it is, nothing below exists.
  // Otherwise ONE launch of input_classes_kernel turns the tick's block into rs_out, which takes the place of the caller's audio in front of
  // conv0.  A uniform engine (vapx_set_input_rate and / or vapx_set_input_format) is the one class cls[0]; an engine with a table
  // (vapx_set_input_classes, cls_table) gives every stream a class of its own
  int n_cls = 0;
  bool cls_table = false;
  InputClassGeom cls[VAPX_MAX_INPUT_CLASSES] = {};
  int tab_cls() const { return cls_table ? n_cls : 0; }               // what the public class calls see: a uniform engine has no classes
  int in_fmt() const { return n_cls && !cls_table ? cls[0].fmt : VAPX_PCM_F32; }
  int in_hz() const {                                                 // 0: no rate of the engine's own (16 kHz, or each class's)
    static const int hz[4] = {0, 8000, 32000, 48000};                 // by ResampleGeom::orig
    return n_cls && !cls_table ? hz[cls[0].orig] : 0;
  }
  int hop_in() const { return cls[0].hop_in; }                        // a uniform engine's samples per channel and tick
  size_t cls_lds = 0;                     // floats of dynamic LDS: the largest window of cls[]
  int rs_rec = 0;                         // floats of a stream's history [2][largest H of cls[]], padded to a multiple of 4; 0: every class is 16 kHz.
                                          // Channel 2 starts H floats in on a uniform engine and at half the record with a table (input_classes.h)
  float* rs_hist = nullptr;               // [max_streams][rs_rec], null with rs_rec = 0
  int* rs_started = nullptr;              // [max_streams * 2] the (stream, channel) has consumed a tick since its reset
  int rs_row = 0;                         // floats of a row of rs_out: hop; L on a uniform 16 kHz engine, which may be stepped with full frames
  float* rs_out = nullptr;                // [max_batch][2][rs_row]
  vapx_input_class cls_pub[VAPX_MAX_INPUT_CLASSES] = {};   // a table as the caller gave it
  std::vector<int32_t> stream_cls;        // a table: [max_streams][2] a (stream, channel)'s class; the host builds the slot descriptors from it
  Staged<int> cls_slots;                  // a table: [max_batch] InputSlot {byte_off, cls} of a step
  std::vector<InputSlot> cls_slots_host;
  size_t cls_row_bytes(int c) const { return (size_t)cls[c].hop_in * (size_t)pcm_bytes_per_sample(cls[c].fmt); }   // one channel's row
  size_t cls_slot_bytes(int c) const { return 2 * cls_row_bytes(c); }
  bool deferred_pending = false;          // the latest step left its overlap groups un-joined (VAPX_DEFER_JOIN)
  std::vector<int32_t> pending_resets;    // vapx_reset_stream requests, applied stream-ordered by the next step
  std::vector<uint32_t> id_stamp;         // duplicate-id check: id_stamp[sid] == id_gen <=> sid already in this batch
  uint32_t id_gen = 0;
  std::vector<int32_t> bad_slots;         // batch slots of the latest host-output step whose results were not finite

  // shared trunk (vapx_attach_trunk): followers take the leader's LSTM outputs instead of running the CPC encoder
  vapx_engine* trunk = nullptr;           // set on a follower
  std::vector<vapx_engine*> followers;    // set on the leader
  bool orphaned = false;                  // follower whose leader was destroyed
  uint64_t tick = 0, followed_tick = 0;
  const int* last_ids = nullptr;          // device ids of the latest step (null = identity)
  // a follower at its own window and / or at 1/R of the leader's rate (mixed trunk groups)
  int R = 1;                              // leader ticks per frame of this follower
  bool own_window = false;                // R == 1, ctx_frames differs from the leader's: bn / bhead from this engine's frames_seen
  std::vector<int32_t> last_ids_host;     // leader: host copy of the latest step's ids (identity spelled out) ...
  bool last_ids_known = false;            // ... unless they were device ids
  std::vector<int32_t> phase;             // R > 1: leader ticks since the stream's last follower frame, per stream
  float *acc = nullptr, *mixA = nullptr, *out_c = nullptr;   // R > 1: TrunkCollectArgs acc / A, compact output rows [max_batch][784]
  Staged<int> mix;                        // R > 1: [3][max_batch] stream id | leader slot | pos of this tick's entries
  std::vector<int> mix_host;              // ... as the host sorts them
  // vapx_step_group (leader only): the tick's wire rows, model-major, on the device and in page-locked host memory
  Staged<float> gw;                       // allocated by the first host-output group step (the follower set is fixed once anyone has stepped)
  std::vector<std::pair<int32_t, int32_t>> group_bad;   // (batch slot, model index) pairs of the latest host-output vapx_step_group
  // vapx_export_streams / vapx_import_streams: ids of up to max_streams streams; bounded staging blocks for host records (allocated
  // on the first host-buffer call; the pinned one only for pageable memory).  vapx_get_state / vapx_set_state move their one record
  // through the same blocks
  Staged<int> sio_ids;
  Staged<float> sio;

  // optional per-kernel-class HIP-event timing (vapx_profile_*): events are recorded on the launch
  // stream around the launches whose class bit is set in prof_mask
  uint32_t prof_mask = 0;
  struct ProfRec { hipEvent_t a, b; int cls; };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> prof_pool;
};

namespace {

int fail(vapx_engine* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  else g_create_error = buf;
  return code;
}

#define HIPCHK(h, expr)                                                                          \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) return fail(h, VAPX_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// free (and null) the buffers of the scratch table: all of them, or the encoder's (what a trunk follower never uses)
void release_scratch(Scratch& sc, bool encoder_only) {
  for (const ScratchRow& r : kScratchTable) {
    if (encoder_only && !r.encoder) continue;
    const ScratchSlot p = r.slot(sc);
    if (p.f) { dfree(*p.f); *p.f = nullptr; }
    else { dfree(*p.i); *p.i = nullptr; }
  }
}

int rate_ok(int hz) { return hz == 5 || hz == 10 || hz == 20 || hz == 50; }

// kernel classes for profiling: 0..4 = GEMM by epilogue (EPI_STORE .. EPI_CN_RELU), then the rest; EPI_BIAS_LN_GELU (= 5 as an epilogue id)
// is booked as class 13 — 5 is the fused conv tail (round 3 booked both under 5: a follower's downsample GEMM was priced as conv_tail)
enum { CLS_CONVTAIL = 5, CLS_FFN = 6, CLS_LASTROW = 7, CLS_CONV0 = 8, CLS_LSTM = 9, CLS_GATHER = 10, CLS_ATTN = 11, CLS_HEAD = 12,
       CLS_GEMM_BIAS_LN_GELU = 13,
       CLS_FFN_PROJ = 14,   // long windows: the mode-2 flat-row block (attention output projection + LN_src + cross-attention query): two
                            // contractions per row where the FFN block proper has seven to twelve — its own class so that a class's
                            // FLOPs, time and HBM bytes describe the same launches (bench.py roofline)
       CLS_TRUNK_COLLECT = 15,   // a slower trunk follower's collect (trunk_collect_kernel) and its output scatter: pure copies
       CLS_COUNT = 16 };
static inline int gemm_class(int epi) { return epi == EPI_BIAS_LN_GELU ? CLS_GEMM_BIAS_LN_GELU : epi; }

struct ProfScope {
  vapx_engine* h; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; int cls;
  ProfScope(vapx_engine* h_, int cls_, hipStream_t st_) : h(h_), st(st_), cls(cls_) {
    if (!(h->prof_mask & (1u << cls))) return;
    auto get = [&]() {
      hipEvent_t e = nullptr;
      if (!h->prof_pool.empty()) { e = h->prof_pool.back(); h->prof_pool.pop_back(); }
      else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
      return e;
    };
    a = get(); b = get();
    if (a) (void)hipEventRecord(a, st);
  }
  ~ProfScope() {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    h->prof_recs.push_back({a, b, cls});
  }
};

// bounded_A: the A operand is bounded by construction (a LayerNorm / ChannelNorm+ReLU output, LSTM outputs): only then may the opt-in
// split-precision product run (f16 operands overflow at 65504); GEMMs on RAW residual-stream / attention rows stay on the fp32 MFMA
hipError_t gemm(vapx_engine* h, const GemmArgs& g, int epi, hipStream_t st, bool bounded_A = true) {
  ProfScope ps(h, gemm_class(epi), st);
  if ((h->cfg.flags & VAPX_FLAG_SPLIT_F16) && bounded_A) {
    GemmArgs gs = g;
    gs.split = 1;
    return launch_gemm_f32(gs, epi, 0, st);
  }
  return launch_gemm_f32(g, epi, 0, st);
}

GemmArgs gemm_args(const float* A, RowMap am, const float* W, int M, int N, int K, float* C, RowMap cm) {
  GemmArgs g;
  memset(&g, 0, sizeof g);
  g.A = A; g.am = am; g.W = W; g.M = M; g.N = N; g.K = K; g.C = C; g.cm = cm;
  g.rm = cm; g.c2m = cm;
  return g;
}

// ---- the CPC encoder between conv0 and the LSTM on B entries: h0 -> gx [B*2][ncpc][1024] (conv1 .. conv4, the LSTM input projection).
// An entry is a stream of a step, or a (frame, stream) pair of vapx_prefill: nothing here knows the difference
int run_conv_chain(vapx_engine* h, const Scratch& sc, int B, hipStream_t st) {
  const int* P = h->P;
  const Weights& w = h->wt;
  struct ConvSpec { const float* in; int Pin, guard_in, k, s; float* out; int Pout, guard_out; };
  const ConvSpec cs[3] = {   // conv1 .. conv3
      {sc.h0, P[0], 2, 8, 4, sc.h1, P[1], 1},
      {sc.h1, P[1], 1, 4, 2, sc.h2, P[2], 1},
      {sc.h2, P[2], 1, 4, 2, sc.h3, P[3], 1},
  };
  // one stream per workgroup pays 27 % row padding: worth it only while the three GEMMs cannot fill the chip
  // (on the split-precision path the three GEMMs are 2x cheaper and beat the fp32 fused tail even at 256 streams)
  const bool fused_tail = conv_tail_supported(P[1], h->ncpc) && !(h->cfg.flags & VAPX_FLAG_UNFUSED_CONV) &&
                          !(h->cfg.flags & VAPX_FLAG_SPLIT_F16) && B <= 512;
  if (fused_tail) h->pass.tail_fused = true;   // B is this group's batch: vapx_peek must not re-derive the decision from the pass's entries
  for (int i = 0; i < (fused_tail ? 1 : 3); ++i) {
    const ConvSpec& c = cs[i];
    const ConvW& cw = w.conv[i + 1];
    RowMap am{(long)(c.Pin + 2 * c.guard_in) * 256, (long)c.s * 256, c.Pout};
    RowMap cm{(long)(c.Pout + 2 * c.guard_out) * 256, 256, c.Pout};
    GemmArgs g = gemm_args(c.in, am, cw.w, B * 2 * c.Pout, 256, c.k * 256, c.out + c.guard_out * 256, cm);
    g.W16 = cw.w16; g.bias = cw.b; g.gamma = cw.g; g.beta = cw.beta;
    HIPCHK(h, gemm(h, g, EPI_CN_RELU, st));
  }
  if (fused_tail) {
    // conv2 -> conv3 -> conv4 for one stream per workgroup, intermediates in LDS
    ConvTailArgs ct;
    ct.h1 = sc.h1; ct.w2f = w.conv[2].wf; ct.w3f = w.conv[3].wf; ct.w4f = w.conv[4].wf;
    ct.b2 = w.conv[2].b; ct.g2 = w.conv[2].g; ct.be2 = w.conv[2].beta;
    ct.b3 = w.conv[3].b; ct.g3 = w.conv[3].g; ct.be3 = w.conv[3].beta;
    ct.b4 = w.conv[4].b; ct.g4 = w.conv[4].g; ct.be4 = w.conv[4].beta;
    ct.z = sc.z; ct.P1 = P[1]; ct.ncpc = h->ncpc;
    { ProfScope ps(h, CLS_CONVTAIL, st); HIPCHK(h, launch_conv_tail(ct, B, st)); }
  } else {  // conv4: only positions 1..P4-2 survive z[:, 1:-1] (encoder.py:76)
    RowMap am{(long)(P[3] + 2) * 256, 2 * 256, h->ncpc};
    GemmArgs g = gemm_args(sc.h3 + 2 * 256, am, w.conv[4].w, B * 2 * h->ncpc, 256, 4 * 256, sc.z, contiguous_rows(256));
    g.W16 = w.conv[4].w16; g.bias = w.conv[4].b; g.gamma = w.conv[4].g; g.beta = w.conv[4].beta;
    HIPCHK(h, gemm(h, g, EPI_CN_RELU, st));
  }
  {  // LSTM input projection for all n_cpc steps at once: gx = z.W_ih^T + (b_ih + b_hh)
    GemmArgs g = gemm_args(sc.z, contiguous_rows(256), w.lstm_wih, B * 2 * h->ncpc, 1024, 256, sc.gx, contiguous_rows(1024));
    g.W16 = w.lstm_wih16; g.bias = w.lstm_b;
    HIPCHK(h, gemm(h, g, EPI_STORE, st));
  }
  return VAPX_OK;
}

// the LSTM's arguments but its batch (M, ids, en): the weights and the buffers of `sc`
void lstm_args(const vapx_engine* h, const Scratch& sc, const StateView& sv, LstmArgs& la) {
  const Weights& w = h->wt;
  la.gx = sc.gx; la.h_state = sv.h_state; la.c_state = sv.c_state;
  la.wfrag = w.lstm_whh; la.out = sc.lstm_out; la.ncpc = h->ncpc;
  // downsample (single-output Conv1d == dense [ncpc*256 -> 256]) + LN + GELU fused into the LSTM kernel
  la.down_wf = w.down_wf; la.down_b = w.down_b; la.down_g = w.down_g; la.down_beta = w.down_beta;
  la.e = sc.e;
  la.ln0_g = h->layer[0].ln_self_g; la.ln0_b = h->layer[0].ln_self_b;
}

// ---- the CPC encoder on B streams: frames -> e [B*2][256] -------------------------------------
int run_encoder(vapx_engine* h, const Scratch& sc, const StateView& sv, int B, const int* ids_dev, const float* audio,
                int spc, bool use_state_meta, hipStream_t st) {
  const Weights& w = h->wt;
  Conv0Args c0;
  c0.audio = audio; c0.ids = ids_dev; c0.carry = use_state_meta ? sv.carry : nullptr;
  c0.h0 = sc.h0; c0.w = w.conv[0].w; c0.bias = w.conv[0].b; c0.gamma = w.conv[0].g; c0.beta = w.conv[0].beta;
  c0.frames_seen = use_state_meta ? sv.frames_seen : nullptr; c0.bn = sc.bn; c0.bhead = sc.bhead;
  c0.L = h->L; c0.spc = spc; c0.T = h->T;
  { ProfScope ps(h, CLS_CONV0, st); HIPCHK(h, launch_conv0(c0, B, st)); }
  { int rc = run_conv_chain(h, sc, B, st); if (rc) return rc; }
  LstmArgs la;
  lstm_args(h, sc, sv, la);
  la.ids = ids_dev; la.M = B * 2; la.en = use_state_meta ? sc.en : nullptr;
  { ProfScope ps(h, CLS_LSTM, st); HIPCHK(h, launch_lstm(la, st)); }
  return VAPX_OK;
}

struct RingView { const float* ring; const float* ring_qkv; const int* ids; };   // layer 0 reads the rings directly
// vapx_transformer_maps: destinations of the attention weights (device, any may be null), each [B][2][layers][4][rows][rows]
struct MapOut { float *attn, *self_attn, *cross_attn; int rows; };

// one run_layers call, as its parts see it
struct LayerRun {
  vapx_engine* h; const Scratch& sc; int B; hipStream_t st; const RingView* rv; const MapOut* maps;
  int T, M;      // window rows; B * 2 * T
  bool split;    // VAPX_FLAG_SPLIT_F16: fp32-accurate products on the f16 matrix cores
};
// what a layer's attention part leaves to its FFN block: null att = xmid is complete (the short-window block and the GEMM chain project and
// normalise themselves); else the block first computes xmid = resid + att . w^T (long window: the projection is fused into the FFN block)
struct AttnOut { const float *att = nullptr, *w = nullptr, *resid = nullptr; bool resid_from_ring = false; };

// maps: one attention_map_kernel launch next to an attention launch, on that launch's own Q and K rows (after their producers, before the
// layer's FFN block overwrites sc.qkv / sc.kvx with the next layer's); no ProfScope: a diagnostic path outside the class table
hipError_t emit_map(const LayerRun& r, int l, bool cross) {
  const MapOut* maps = r.maps;
  const Scratch& sc = r.sc;
  float* dst = !maps ? nullptr : cross ? maps->cross_attn : l == 0 ? maps->attn : maps->self_attn;
  if (!dst || (cross && l == 0)) return hipSuccess;
  const long rr = (long)maps->rows * maps->rows;
  const int n_layers = l == 0 ? 1 : 3, li = l == 0 ? 0 : l - 1;
  AttnMapArgs ma{cross ? sc.qx : sc.qkv, cross ? sc.kvx : sc.qkv + 256, sc.bn, r.T, cross ? 256 : 768, cross ? 512 : 768, cross ? 1 : 0,
                 dst + li * 4 * rr, n_layers * 4 * rr, rr, maps->rows};
  return launch_attention_map(ma, r.B, r.st);
}

// the stand-alone attention kernel of a long window: split-precision up to 256 rows, else fp32 (attention_xl_kernel when forced or needed)
hipError_t launch_attn(vapx_engine* h, const AttnArgs& a, int B, hipStream_t st) {
  ProfScope ps(h, CLS_ATTN, st);
  return (h->cfg.flags & VAPX_FLAG_SPLIT_F16) && h->T <= 256 ? launch_attention_f16x3(a, B, st) : launch_attention(a, B, st, h->force_xl);
}

// T <= 64, fused: attention + output projection + residual + LayerNorm (+ cross-attention queries)
int attn_short(const LayerRun& r, int l, AttnOut*) {
  vapx_engine* h = r.h; const Scratch& sc = r.sc; const int B = r.B, T = r.T; hipStream_t st = r.st; const RingView* rv = r.rv;
  const Layer& Lw = h->layer[l];
  const float* xin = sc.xl[l];
  AttnBlockArgs ab;
  memset(&ab, 0, sizeof ab);
  ab.q = sc.qkv; ab.k = sc.qkv + 256; ab.v = sc.qkv + 512; ab.ldq = 768; ab.ldkv = 768; ab.swap_kv = 0;
  const bool asplit = r.split;
  ab.split = asplit ? 1 : 0;
  ab.bn = sc.bn; ab.T = T; ab.wprojf = asplit ? Lw.wprojh : Lw.wprojf; ab.resid = xin; ab.xmid = sc.xmid;
  if (l == 0 && rv && rv->ring) {   // Q|K|V and the residual straight from the per-stream rings
    ab.q = rv->ring_qkv; ab.k = rv->ring_qkv + 256; ab.v = rv->ring_qkv + 512; ab.resid = rv->ring;
    ab.ring_rot = sc.rot; ab.ids = rv->ids;
  }
  if (l == 0) { ab.ln_g = Lw.ln_ffn_g; ab.ln_b = Lw.ln_ffn_b; }
  else { ab.ln_g = Lw.ln_src_g; ab.ln_b = Lw.ln_src_b; ab.wqxf = asplit ? Lw.wqxh : Lw.wqxf; ab.qx = sc.qx; }
#ifdef VAPX_TRACE
  if (h->attn_trace && l == 1 && (size_t)B * 2 <= 16384) { ab.trace = h->attn_trace; h->attn_trace_wgs = (size_t)B * 2; }
#endif
  { ProfScope ps(h, CLS_ATTN, st); HIPCHK(h, launch_attn_block(ab, B, st)); }
#ifdef VAPX_TRACE
  ab.trace = nullptr;
#endif
  if (r.maps) { HIPCHK(h, emit_map(r, l, false)); HIPCHK(h, emit_map(r, l, true)); }   // sc.qx: written by the launch above
  if (l > 0) {
    ab.q = sc.qx; ab.k = sc.kvx; ab.v = sc.kvx + 256; ab.ldq = 256; ab.ldkv = 512; ab.swap_kv = 1;
    ab.wprojf = asplit ? Lw.wprojxh : Lw.wprojxf; ab.resid = sc.xmid; ab.ln_g = Lw.ln_ffn_g; ab.ln_b = Lw.ln_ffn_b;
    ab.wqxf = nullptr; ab.qx = nullptr; ab.ring_rot = nullptr; ab.ids = nullptr;
    { ProfScope ps(h, CLS_ATTN, st); HIPCHK(h, launch_attn_block(ab, B, st)); }
  }
  return VAPX_OK;
}

// long window: plain attention kernels; every projection rides in a fused flat-row block (no [rows x 256] GEMM launches).
// xn_ready: sc.xn holds LN_self(layer l)(x) of every row, sc.qkv does NOT hold this layer's Q|K|V
int attn_long_fused(const LayerRun& r, int l, bool xn_ready, AttnOut* out) {
  vapx_engine* h = r.h; const Scratch& sc = r.sc; const int B = r.B, T = r.T; hipStream_t st = r.st; const RingView* rv = r.rv;
  const bool split = r.split;
  const Layer& Lw = h->layer[l];
  const float* xin = sc.xl[l];
  AttnArgs aa{sc.qkv, sc.qkv + 256, sc.qkv + 512, sc.att, sc.bn, T, 768, 768, 0};
  const bool ring0 = l == 0 && rv && rv->ring;
  if (ring0) {   // Q|K|V straight from the per-stream rings (no chronological gather)
    aa.q = rv->ring_qkv; aa.k = rv->ring_qkv + 256; aa.v = rv->ring_qkv + 512;
    aa.ring_rot = sc.rot; aa.ids = rv->ids;
  }
  const bool proj_here = xn_ready && l > 0 && Lw.wqkvp;
#ifdef VAPX_TRACE
  if (h->attn_trace && l == 1) { aa.trace = h->attn_trace; h->attn_trace_wgs = std::min<size_t>(16384, (size_t)B * 8); }
#endif
  if (proj_here) {
    AttnProjArgs ap{sc.xn, Lw.wqkvp, sc.att, sc.bn, T, 0};
    ProfScope ps(h, CLS_ATTN, st);
    HIPCHK(h, launch_attention_proj_f16x3(ap, B, st));
  } else {
    HIPCHK(h, launch_attn(h, aa, B, st));
  }
  if (r.maps) HIPCHK(h, emit_map(r, l, false));
  out->att = sc.att; out->w = split ? Lw.wproj8 : Lw.wprojf; out->resid = ring0 ? rv->ring : xin;
  out->resid_from_ring = ring0;
  if (l > 0) {
    // self half: xmid = xin + att.Wproj^T ; qx = LN_src(xmid).Wq_x^T
    FfnArgs fp;
    memset(&fp, 0, sizeof fp);
    fp.mode = 2; fp.M = r.M; fp.att = sc.att; fp.wprojf = split ? Lw.wproj8 : Lw.wprojf; fp.resid = xin; fp.xmid_out = sc.xmid;
    fp.ln_g = Lw.ln_src_g; fp.ln_b = Lw.ln_src_b; fp.wqkvf = split ? Lw.wqx8 : Lw.wqxf; fp.n_qkv_chunks = 1; fp.qkv = sc.qx;
    { ProfScope ps(h, CLS_FFN_PROJ, st); HIPCHK(h, split ? launch_ffn_block_f16x3(fp, st) : launch_ffn_block(fp, st)); }
    AttnArgs ax{sc.qx, sc.kvx, sc.kvx + 256, sc.att, sc.bn, T, 256, 512, 1};
    HIPCHK(h, launch_attn(h, ax, B, st));
    if (r.maps) HIPCHK(h, emit_map(r, l, true));
    out->w = split ? Lw.wprojx8 : Lw.wprojxf; out->resid = sc.xmid;
  }
  return VAPX_OK;
}

// long window, VAPX_FLAG_UNFUSED_PROJ: attention kernels with stand-alone projection GEMMs
int attn_gemm_chain(const LayerRun& r, int l, AttnOut*) {
  vapx_engine* h = r.h; const Scratch& sc = r.sc; const int B = r.B, T = r.T, M = r.M; hipStream_t st = r.st;
  const RowMap r256 = contiguous_rows(256);
  const Layer& Lw = h->layer[l];
  const float* xin = sc.xl[l];
  // self attention
  AttnArgs aa{sc.qkv, sc.qkv + 256, sc.qkv + 512, sc.att, sc.bn, T, 768, 768, 0};
  HIPCHK(h, launch_attn(h, aa, B, st));
  if (r.maps) HIPCHK(h, emit_map(r, l, false));
  GemmArgs g = gemm_args(sc.att, r256, Lw.wproj, M, 256, 256, sc.xmid, r256);
  g.resid = xin; g.C2 = sc.xn;
  if (l == 0) { g.gamma = Lw.ln_ffn_g; g.beta = Lw.ln_ffn_b; }
  else { g.gamma = Lw.ln_src_g; g.beta = Lw.ln_src_b; }
  HIPCHK(h, gemm(h, g, EPI_RESID_LN, st, /*bounded_A=*/false));   // raw attention rows
  if (l > 0) {
    // cross attention: Q from LN_src(x), K/V from the OTHER channel's raw layer input
    g = gemm_args(sc.xn, r256, Lw.wq_x, M, 256, 256, sc.qx, r256);
    HIPCHK(h, gemm(h, g, EPI_STORE, st));
    AttnArgs ax{sc.qx, sc.kvx, sc.kvx + 256, sc.att, sc.bn, T, 256, 512, 1};
    HIPCHK(h, launch_attn(h, ax, B, st));
    if (r.maps) HIPCHK(h, emit_map(r, l, true));
    g = gemm_args(sc.att, r256, Lw.wproj_x, M, 256, 256, sc.xmid, r256);
    g.resid = sc.xmid; g.C2 = sc.xn; g.gamma = Lw.ln_ffn_g; g.beta = Lw.ln_ffn_b;
    HIPCHK(h, gemm(h, g, EPI_RESID_LN, st, /*bounded_A=*/false));
  }
  return VAPX_OK;
}

// ---- layer 3 on the newest row of every (stream, channel) only; K/V (all rows) came from the
//      previous layer's FFN block: sc.qkv = [K | V] [M][512], sc.kvx = cross [K | V] [M][512] ----
int run_last_row(vapx_engine* h, const Scratch& sc, int B, hipStream_t st) {
  const int T = h->T;
  const RowMap r256 = contiguous_rows(256), r768 = contiguous_rows(768);
  const Layer& Lw = h->layer[3];
  const int Ml = B * 2;
  if (!(h->cfg.flags & VAPX_FLAG_UNFUSED_LAST_ROW)) {
    LastBlockArgs lb;
    lb.x = sc.xl[3]; lb.xn = sc.xn; lb.bn = sc.bn; lb.wf = h->wt.l3_last16;
    lb.ln_src_g = Lw.ln_src_g; lb.ln_src_b = Lw.ln_src_b;
    lb.ln_ffn_g = Lw.ln_ffn_g; lb.ln_ffn_b = Lw.ln_ffn_b; lb.out = sc.last[5]; lb.B = B; lb.T = T;
    ProfScope ps(h, CLS_LASTROW, st);
    HIPCHK(h, launch_last_block(lb, st));
    return VAPX_OK;
  }
  float *lx = sc.last[0], *lxn = sc.last[1], *lq = sc.last[2], *latt = sc.last[3], *lxmid = sc.last[4], *lout = sc.last[5];
  ProfScope ps(h, CLS_LASTROW, st);
  LastRowArgs lr{sc.xl[3], sc.bn, lx, lxn, Lw.ln_self_g, Lw.ln_self_b, B, T};
  HIPCHK(h, launch_gather_last_ln(lr, st));
  GemmArgs g = gemm_args(lxn, r256, Lw.wqkv, Ml, 256, 256, lq, r256);            // Q rows of Wqkv
  HIPCHK(h, launch_gemm_f32(g, EPI_STORE, 0, st));
  AttnArgs aa{lq, sc.qkv, sc.qkv + 256, latt, sc.bn, T, 256, 512, 0};
  HIPCHK(h, launch_attention_last(aa, B, st));
  g = gemm_args(latt, r256, Lw.wproj, Ml, 256, 256, lxmid, r256);
  g.resid = lx; g.C2 = lxn; g.gamma = Lw.ln_src_g; g.beta = Lw.ln_src_b;
  HIPCHK(h, launch_gemm_f32(g, EPI_RESID_LN, 0, st));
  g = gemm_args(lxn, r256, Lw.wq_x, Ml, 256, 256, lq, r256);
  HIPCHK(h, launch_gemm_f32(g, EPI_STORE, 0, st));
  AttnArgs ax{lq, sc.kvx, sc.kvx + 256, latt, sc.bn, T, 256, 512, 1};
  HIPCHK(h, launch_attention_last(ax, B, st));
  g = gemm_args(latt, r256, Lw.wproj_x, Ml, 256, 256, lxmid, r256);
  g.resid = lxmid; g.C2 = lxn; g.gamma = Lw.ln_ffn_g; g.beta = Lw.ln_ffn_b;
  HIPCHK(h, launch_gemm_f32(g, EPI_RESID_LN, 0, st));
  // FFN on 2B rows: two plain GEMMs spread over more workgroups than one fused 32-row block would
  g = gemm_args(lxn, r256, Lw.w0, Ml, 768, 256, sc.lffn, r768);
  HIPCHK(h, launch_gemm_f32(g, EPI_GELU, 0, st));
  g = gemm_args(sc.lffn, r768, Lw.w3, Ml, 256, 768, lout, r256);
  g.resid = lxmid;
  HIPCHK(h, launch_gemm_f32(g, EPI_RESID, 0, st));
  return VAPX_OK;
}

// ---- 1 self + 3 self/cross layers on x0 = xl[l_begin] (LN_self already in xn) ---------------------
// Per layer: [QKV (+cross KV) projections] -> self-attention -> proj+residual+LN -> (cross: q GEMM,
// cross-attention, proj+residual+LN) -> fused FFN block, which also emits the NEXT layer's
// projections so that only the first executed layer needs stand-alone projection GEMMs.
int run_layers(vapx_engine* h, const Scratch& sc, int B, hipStream_t st, int l_begin = 0, int l_end = 4,
               bool prune_last = false, bool qkv0_ready = false, const RingView* rv = nullptr, const MapOut* maps = nullptr) {
  const int T = h->T;
  if (maps && (rv || prune_last)) return fail(h, VAPX_E_INVAL, "attention maps need chronological buffers and every row of every layer");
  const int M = B * 2 * T;
  const bool split = (h->cfg.flags & VAPX_FLAG_SPLIT_F16) != 0;
  const LayerRun r{h, sc, B, st, rv, maps, T, M, split};
  const RowMap r256 = contiguous_rows(256), r768 = contiguous_rows(768), r512 = contiguous_rows(512);
  if (prune_last && (l_end != 4 || l_begin > 2)) prune_last = false;
  const int l_full_end = prune_last ? 3 : l_end;
  // split path, long windows: the self-attention of a layer whose LN_self rows were written by the previous layer's flat-row block projects
  // its own Q|K|V (attention_proj_f16x3_kernel); that block then skips the three contractions and never writes sc.qkv
  // (windows of 257 .. 512 frames: attention_xl_kernel — fp32, Q|K|V from the flat-row blocks — on both paths)
  // (a call that wants the self-attention maps needs Q and K in HBM: it takes the VAPX_FLAG_SPLIT_QKV_IN_FFN routing for that call)
  const bool qkv_in_attn = split && !(h->cfg.flags & (VAPX_FLAG_SPLIT_QKV_IN_FFN | VAPX_FLAG_UNFUSED_PROJ)) && T > 64 && T <= 256 &&
                           !(maps && maps->self_attn);
  bool xn_ready = false;                   // sc.xn holds LN_self(layer l)(x) of every row, sc.qkv does NOT hold this layer's Q|K|V
  for (int l = l_begin; l < l_full_end; ++l) {
    const Layer& Lw = h->layer[l];
    if (l == l_begin && !(l == 0 && qkv0_ready)) {
      GemmArgs g = gemm_args(sc.xn, r256, Lw.wqkv, M, 768, 256, sc.qkv, r768);
      HIPCHK(h, gemm(h, g, EPI_STORE, st));
      if (l > 0) {
        g = gemm_args(sc.xl[l], r256, Lw.wkv_x, M, 512, 256, sc.kvx, r512);
        HIPCHK(h, gemm(h, g, EPI_STORE, st, /*bounded_A=*/false));   // raw residual rows
      }
    }
    AttnOut pre;
    const int rc = T <= 64 ? attn_short(r, l, &pre)
                 : !(h->cfg.flags & VAPX_FLAG_UNFUSED_PROJ) ? attn_long_fused(r, l, xn_ready, &pre) : attn_gemm_chain(r, l, &pre);
    if (rc) return rc;
    // feed-forward (+ next layer's projections)
    FfnArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.xmid = sc.xmid; fa.lnf_g = Lw.ln_ffn_g; fa.lnf_b = Lw.ln_ffn_b; fa.xout = sc.xl[l + 1]; fa.M = M;
    if (pre.att) { fa.mode = 1; fa.att = pre.att; fa.wprojf = pre.w; fa.resid = pre.resid; fa.xmid_out = sc.xmid; }
    if (pre.resid_from_ring) { fa.resid_rot = sc.rot; fa.resid_ids = rv->ids; fa.resid_T = T; }
    fa.w0f = split ? Lw.w0h : Lw.w0f; fa.w3f = split ? Lw.w3h : Lw.w3f; fa.hid_scale = Lw.hid_scale;
    xn_ready = false;
    if (l + 1 < l_end) {
      const Layer& Ln = h->layer[l + 1];
      const float* nqkv = split ? Ln.wqkvh : Ln.wqkvf;
      fa.ln_g = Ln.ln_self_g; fa.ln_b = Ln.ln_self_b; fa.wqkvf = nqkv; fa.qkv = sc.qkv; fa.n_qkv_chunks = 3;
      fa.wkvxf = split ? Ln.wkvxh : Ln.wkvxf; fa.kvx = sc.kvx;
      if (qkv_in_attn && pre.att && Ln.wqkvp && !(prune_last && l + 1 == 3)) {   // the next layer's self-attention projects Q|K|V itself
        fa.wqkvf = nullptr; fa.n_qkv_chunks = 0; fa.xn_out = sc.xn;
        xn_ready = true;
      }
      if (prune_last && l + 1 == 3) {
        if (h->cfg.flags & VAPX_FLAG_UNFUSED_LAST_ROW) {   // the pruned layer needs K,V of every row but Q of one row only
          fa.wqkvf = nqkv + 65536; fa.n_qkv_chunks = 2;
        } else {   // fused last-row block: K / V projections are absorbed into the single query (csrc/last_block.hip);
                   // it only needs LN_self(x) of every row next to the raw rows
          fa.wqkvf = nullptr; fa.n_qkv_chunks = 0; fa.wkvxf = nullptr; fa.xn_out = sc.xn;
        }
      }
    }
#ifdef VAPX_TRACE
    if (h->ffn_trace && l == 0) {
      fa.trace = h->ffn_trace;
      h->ffn_trace_wgs = std::min<size_t>(16384, (size_t)(M + 31) / 32);
      if ((size_t)(M + 31) / 32 > 16384) fa.trace = nullptr;
    }
#endif
    { ProfScope ps(h, CLS_FFN, st); HIPCHK(h, split ? launch_ffn_block_f16x3(fa, st) : launch_ffn_block(fa, st)); }
  }
  return prune_last ? run_last_row(h, sc, B, st) : VAPX_OK;
}

// nod variant: p_bc = sigmoid(bc_head(comb)) for EVERY row of the window (vap_nod_main.py:276 indexes the
// batch dim, so all n rows are emitted); one wave per (stream, row); written over the (unused in
// nod mode) logits slots of the output row.
__global__ void pbc_rows_kernel(const float* comb, const float* w, const float* bias, const int* bn, float* out,
                                int B, int T, int out_stride) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * T) return;
  const int b = (int)(row / T), t = (int)(row - (long)b * T);
  float v = 0.f;
  if (t < bn[b]) {
    f32x4 x = *(const f32x4*)(comb + row * 256 + lane * 4), ww = *(const f32x4*)(w + lane * 4);
    float d = wave_sum(x[0] * ww[0] + x[1] * ww[1] + x[2] * ww[2] + x[3] * ww[3]);
    v = 1.0f / (1.0f + expf(-(d + bias[0])));
  }
  if (lane == 0 && t < 256) out[(long)b * out_stride + VAPX_OUT_LOGITS + t] = v;
}

__global__ void fill_int_kernel(int* p, int v, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// stream-ordered reset of up to 16 stream slots: LSTM h/c, carry and window fill back to zero (the rings need no
// clearing: rows beyond frames_seen are never read).  One workgroup per slot.
struct ResetList { int n; int ids[16]; int* fs[4]; };   // fs[0] = this engine's frames_seen, fs[1..] = trunk followers'
// ids[k] < 0 encodes "carry only" for stream -ids[k] - 1 (what a reconnect does in the reference, vap_main.py:368-369)
// an engine with an input rate: the resampler history goes with the carry (a new connection is a new signal)
__global__ void reset_streams_kernel(ResetList r, float* h_state, float* c_state, float* carry, float* rs_hist, int* rs_started, int rs_rec) {
  const int raw = r.ids[blockIdx.x];
  const bool carry_only = raw < 0;
  const int sid = carry_only ? -raw - 1 : raw;
  for (int i = threadIdx.x; i < 2 * VAPX_PAD; i += blockDim.x) carry[(long)sid * 2 * VAPX_PAD + i] = 0.f;
  if (rs_hist) {
    for (int i = threadIdx.x; i < rs_rec; i += blockDim.x) rs_hist[(long)sid * rs_rec + i] = 0.f;
    if (threadIdx.x < 2) rs_started[sid * 2 + threadIdx.x] = 0;
  }
  if (carry_only) return;
  for (int i = threadIdx.x; i < 512; i += blockDim.x) { h_state[(long)sid * 512 + i] = 0.f; c_state[(long)sid * 512 + i] = 0.f; }
  if (threadIdx.x < 4 && r.fs[threadIdx.x]) r.fs[threadIdx.x][sid] = 0;
}
__global__ void add_kernel(float* o, const float* a, const float* b, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}
// ---- level-1 head surface (vap_main.py:290-307 calls these on tensors of ANY row count): one wave per row ----
// y[r] = x[r] . w + b                                   (va_classifier: Linear(256, 1), vap_main.py:142,292-293)
__global__ void rowdot_kernel(const float* x, const float* w, const float* bias, float* y, long rows) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  f32x4 xv = *(const f32x4*)(x + r * 256 + lane * 4), wv = *(const f32x4*)(w + lane * 4);
  const float d = wave_sum(xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3]);
  if (lane == 0) y[r] = d + bias[0];
}
// y[r][o] = x[r] . w[o] + b[o], o < nout <= 4   (bc_head: Linear(256, 3) / Linear(256, 1), nod_head: Linear(256, 4);
// vap_realtime/vap_models.py:220,328-329, applied to out["x"] of ANY row count at vap_realtime/model.py:197,217-218)
__global__ void rowheads_kernel(const float* x, const float* w, const float* bias, float* y, long rows, int nout) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const f32x4 xv = *(const f32x4*)(x + r * 256 + lane * 4);
  for (int o = 0; o < nout; ++o) {
    const f32x4 wv = *(const f32x4*)(w + o * 256 + lane * 4);
    const float d = wave_sum(xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3]);
    if (lane == 0) y[r * nout + o] = d + bias[o];
  }
}
// softmax over the 256 classes of a row (probs = logits.softmax(-1), vap_main.py:295)
__global__ void softmax256_kernel(const float* x, float* y, long rows) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  f32x4 v = *(const f32x4*)(x + r * 256 + lane * 4);
  const float mx = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  f32x4 e = {expf(v[0] - mx), expf(v[1] - mx), expf(v[2] - mx), expf(v[3] - mx)};
  const float inv = 1.0f / wave_sum(e[0] + e[1] + e[2] + e[3]);
  *(f32x4*)(y + r * 256 + lane * 4) = e * inv;
}
// ObjectiveVAP.probs_next_speaker_aggregate (objective.py:186-206): class i <-> 8 bits, speaker c owns bits 4c..4c+3;
// p[c] = sum_i probs[i] * #set bits of i among bins [from, to] of speaker c;  p /= p0 + p1 + 1e-5
__global__ void aggregate_kernel(const float* probs, float* out, long rows, int from_bin, int to_bin) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  f32x4 p = *(const f32x4*)(probs + r * 256 + lane * 4);
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = lane * 4 + u;
    int c0 = 0, c1 = 0;
    for (int b = from_bin; b <= to_bin; ++b) { c0 += (i >> b) & 1; c1 += (i >> (4 + b)) & 1; }
    a0 += p[u] * (float)c0;
    a1 += p[u] * (float)c1;
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  if (lane == 0) { const float d = a0 + a1 + 1e-5f; out[r * 2] = a0 / d; out[r * 2 + 1] = a1 / d; }
}

// compact [B*2][T][256] scratch rows (t < rows) into [B*2][rows][256]
__global__ void compact_rows_kernel(float* dst, const float* src, int T, int rows, long nrows_out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
  if (i >= nrows_out * 64) return;
  long r = i >> 6;
  int q = (int)(i & 63);
  long bc = r / rows;
  int t = (int)(r - bc * rows);
  ((f32x4*)dst)[i] = ((const f32x4*)src)[(bc * T + t) * 64 + q];
}

// host stream ids of one call: in range and distinct
int check_ids(vapx_engine* h, int n, const int32_t* ids) {
  if (++h->id_gen == 0) { std::fill(h->id_stamp.begin(), h->id_stamp.end(), 0u); h->id_gen = 1; }
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id %d out of range [0,%d)", ids[i], h->cfg.max_streams);
    // two batch slots on one stream would race on its ring slot, LSTM state, carry and frame counter
    if (h->id_stamp[ids[i]] == h->id_gen) return fail(h, VAPX_E_INVAL, "stream id %d appears twice in one call (batch slot %d)", ids[i], i);
    h->id_stamp[ids[i]] = h->id_gen;
  }
  return VAPX_OK;
}

// a call's stream ids on the device: host ids (check_ids has passed them) travel through `buf`; device ids and none (identity) stay
int upload_ids(vapx_engine* h, Staged<int>& buf, int n, const int32_t* ids, int flags, hipStream_t st, const int** out) {
  *out = ids;
  if (!ids || (flags & VAPX_IDS_DEVICE)) return VAPX_OK;
  HIPCHK(h, buf.upload(ids, n, st));
  *out = buf.dev;
  return VAPX_OK;
}

// apply the vapx_reset_stream requests collected since the last step, ordered on `st` (no host or device sync)
int flush_resets(vapx_engine* h, hipStream_t st) {
  if (h->pending_resets.empty()) return VAPX_OK;
  ResetList r;
  memset(&r, 0, sizeof r);
  r.fs[0] = h->frames_seen;
  size_t nf = 0;
  for (vapx_engine* f : h->followers)
    if (nf + 1 < 4) r.fs[++nf] = f->frames_seen;   // a fourth and later follower gets its own tiny launches below
  for (size_t i = 0; i < h->pending_resets.size(); i += 16) {
    r.n = (int)std::min<size_t>(16, h->pending_resets.size() - i);
    for (int k = 0; k < r.n; ++k) r.ids[k] = h->pending_resets[i + k];
    hipLaunchKernelGGL(reset_streams_kernel, dim3(r.n), dim3(256), 0, st, r, h->h_state, h->c_state, h->carry, h->rs_hist, h->rs_started, h->rs_rec);
    for (size_t f = 3; f < h->followers.size(); ++f)
      for (int k = 0; k < r.n; ++k)
        if (r.ids[k] >= 0) hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64), 0, st, h->followers[f]->frames_seen + r.ids[k], 0, 1);
  }
  HIPCHK(h, hipGetLastError());
  for (vapx_engine* f : h->followers)   // a slower follower starts the stream's next frame from its first leader hop (acc needs no clearing)
    if (f->R > 1)
      for (int32_t q : h->pending_resets)
        if (q >= 0) f->phase[q] = 0;
  h->pending_resets.clear();
  return VAPX_OK;
}

// Every call that takes an engine runs in one order: its argument checks (host stream ids among them: check_ids) before anything is
// enqueued, then enter(), then - where it touches stream state or the scratch buffers - settle() or, synchronising, quiesce().
//
// enter: a stale error of an earlier, unrelated HIP call (this library's or anyone's) is not this call's, and the device is the engine's
int enter(vapx_engine* h) {
  (void)hipGetLastError();
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return VAPX_OK;
}

// make `st` wait for overlap groups a VAPX_DEFER_JOIN step left running
int join_deferred(vapx_engine* h, hipStream_t st) {
  if (!h->deferred_pending) return VAPX_OK;
  for (int g = 0; g < h->pass.groups; ++g) HIPCHK(h, hipStreamWaitEvent(st, h->gdone[g], 0));
  h->deferred_pending = false;
  return VAPX_OK;
}

// settle: order `st` behind this engine's un-joined overlap groups and apply the queued resets.  They live in the trunk leader and touch
// every engine of its group (a follower's head_kernel writes the frame counter the reset zeroes), so with resets queued the leader's and
// every follower's groups are joined before the leader's reset kernel goes to `st`
int settle(vapx_engine* h, hipStream_t st) {
  int rc = join_deferred(h, st);
  vapx_engine* lead = h->trunk ? h->trunk : h;
  if (rc || lead->pending_resets.empty()) return rc;
  if ((rc = join_deferred(lead, st))) return rc;
  for (vapx_engine* f : lead->followers)
    if ((rc = join_deferred(f, st))) return rc;
  rc = flush_resets(lead, st);
  return rc == VAPX_OK || h == lead ? rc : fail(h, rc, "trunk leader: %s", lead->err.c_str());
}
int enter_settled(vapx_engine* h, hipStream_t st) {
  const int rc = enter(h);
  return rc ? rc : settle(h, st);
}

// the synchronising form (vapx_get_state / vapx_set_state, peeks): the device idle, the queued resets applied
int quiesce(vapx_engine* h) {
  if (int rc = enter(h)) return rc;
  HIPCHK(h, hipDeviceSynchronize());
  vapx_engine* lead = h->trunk ? h->trunk : h;
  if (!lead->pending_resets.empty()) {
    int rc = flush_resets(lead, nullptr);
    if (rc) return rc;
    HIPCHK(h, hipDeviceSynchronize());
  }
  h->deferred_pending = false;
  return VAPX_OK;
}

// Combinator on ALL rows: comb = gelu(LN(a.Wa^T)) + gelu(LN(b.Wb^T)), shared LN (modules.py:449-464).
// Tower rows of channel c of stream b sit at ((b*2+c)*T + t).  Result in sc.xmid as [n][T][256].
int run_combinator_all_rows(vapx_engine* h, const Scratch& sc, int n, hipStream_t st) {
  const int T = h->T, M = n * T;
  for (int c = 0; c < 2; ++c) {
    RowMap am{(long)2 * T * 256, 256, T};
    GemmArgs g = gemm_args(sc.xl[4] + (long)c * T * 256, am, c ? h->wt.comb_wb : h->wt.comb_wa, M, 256, 256,
                           c ? sc.qx : sc.att, contiguous_rows(256));
    g.gamma = h->wt.comb_g; g.beta = h->wt.comb_b;
    HIPCHK(h, gemm(h, g, EPI_BIAS_LN_GELU, st, /*bounded_A=*/false));   // raw last-layer rows
  }
  const long tot = (long)M * 256;
  hipLaunchKernelGGL(add_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, sc.xmid, sc.att, sc.qx, tot);
  return VAPX_OK;
}

// one sub-batch of a tick: encoder -> ring -> transformer -> heads.  `b0` is the offset of the
// group inside the caller's batch (identity stream ids when ids == nullptr start at b0).
int step_group(vapx_engine* h, const Scratch& sc_own, int nb, int b0, const int* ids, const float* audio, int spc,
               float* out, hipStream_t st, const Scratch* lead = nullptr) {
  Scratch sc = sc_own;
  // window fill / ring slot: decided by the leader's conv0 — unless this follower keeps a window or a rate of its own
  if (lead && !h->own_window && h->R == 1) { sc.bn = lead->bn; sc.bhead = lead->bhead; }
  // identity ids: kernels index state by batch slot, so advance the state bases by b0 streams
  const size_t s0 = ids ? 0 : (size_t)b0;
  const StateView sv{h->ring + s0 * 2 * h->T * 256, h->ring_qkv + s0 * 2 * h->T * 768, h->h_state + s0 * 512, h->c_state + s0 * 512,
                     h->carry + s0 * 2 * VAPX_PAD, h->frames_seen + s0};
  int rc = VAPX_OK;
  if (!lead) {
    rc = run_encoder(h, sc, sv, nb, ids, audio, spc, true, st);
    if (rc) return rc;
  } else {
    if (h->own_window) HIPCHK(h, launch_window_meta(ids, sv.frames_seen, h->T, sc.bn, sc.bhead, nb, st));
    // this weight set's own downsample on the shared LSTM outputs: e = gelu(LN(Conv1d_K(lstm_out))), en = LN0(e)
    GemmArgs g = gemm_args(lead->lstm_out, contiguous_rows(h->ncpc * 256), h->wt.down_w, nb * 2, 256, h->ncpc * 256, sc.e,
                           contiguous_rows(256));
    g.bias = h->wt.down_b; g.gamma = h->wt.down_g; g.beta = h->wt.down_beta;
    HIPCHK(h, gemm(h, g, EPI_BIAS_LN_GELU, st));
    HIPCHK(h, launch_ln_rows(sc.e, sc.en, h->layer[0].ln_self_g, h->layer[0].ln_self_b, nb * 2, st));
  }
  {  // layer-0 Q|K|V of the NEW row only: they are per-row functions of the embedding, so the other
     // rows' values are cached next to the ring (exact; saves the [rows x 768] GEMM every tick)
    GemmArgs g = gemm_args(sc.en, contiguous_rows(256), h->layer[0].wqkv, nb * 2, 768, 256, sc.qkv_new, contiguous_rows(768));
    g.W16 = h->wt.l0_wqkv16;
    HIPCHK(h, gemm(h, g, EPI_STORE, st));
  }
  GatherArgs ga;
  memset(&ga, 0, sizeof ga);
  ga.ring = sv.ring; ga.ring_qkv = sv.ring_qkv; ga.qkv_new = sc.qkv_new; ga.qkv = sc.qkv;
  ga.e = sc.e; ga.xin = nullptr; ga.ids = ids; ga.bn = sc.bn; ga.bhead = sc.bhead;
  ga.x0 = sc.xl[0]; ga.xn = sc.xn; ga.gamma = h->layer[0].ln_self_g; ga.beta = h->layer[0].ln_self_b;
  ga.B = nb; ga.T = h->T; ga.rows_in = 0;
  const bool ring_direct = h->ring_direct, prune = h->prune_last;
  ga.rot = sc.rot;
  { ProfScope ps(h, CLS_GATHER, st); HIPCHK(h, ring_direct ? launch_ring_append(ga, st) : launch_gather_ln(ga, st)); }
  RingView rv{ring_direct ? sv.ring : nullptr, sv.ring_qkv, ids};
  rc = run_layers(h, sc, nb, st, 0, 4, prune, /*qkv0_ready=*/true, ring_direct ? &rv : nullptr);
  if (rc) return rc;
  HeadArgs ha;
  ha.x = prune ? sc.last[5] : sc.xl[4]; ha.x_last_only = prune ? 1 : 0; ha.o = sc.xl[1]; ha.e = sc.e; ha.bn = sc.bn; ha.ids = ids; ha.frames_seen = sv.frames_seen;
  const Weights& w = h->wt;
  ha.waT = w.comb_waT; ha.wbT = w.comb_wbT; ha.cg = w.comb_g; ha.cb = w.comb_b;
  ha.hwT = w.head_wT; ha.hb = w.head_b; ha.vw = w.vad_w; ha.vb = w.vad_b;
  ha.aw = w.aux_w; ha.ab = w.aux_b; ha.out = out; ha.B = nb; ha.T = h->T; ha.mode = h->cfg.mode;
  ha.out_stride = VAPX_OUT_STRIDE;
  { ProfScope ps(h, CLS_HEAD, st); HIPCHK(h, launch_head(ha, st)); }
  if (h->cfg.mode == VAPX_MODE_NOD) {
    rc = run_combinator_all_rows(h, sc, nb, st);
    if (rc) return rc;
    const long rows = (long)nb * h->T;
    hipLaunchKernelGGL(pbc_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, sc.xmid, w.aux_w + 4 * 256,
                       w.aux_b + 4, sc.bn, out, nb, h->T, VAPX_OUT_STRIDE);
    HIPCHK(h, hipGetLastError());
  }
  return VAPX_OK;
}

}  // namespace

extern "C" {

int32_t vapx_abi_version(void) { return VAPX_ABI_VERSION; }

size_t vapx_blob_floats(int32_t frame_hz) {
  if (!rate_ok(frame_hz)) return 0;
  size_t n = 0;
  const vapx_layout::Entry* lay = vapx_layout::layout_for_K(geometry(frame_hz).ncpc, &n);
  if (!lay) return 0;
  return lay[n - 1].off;  // "__total__"
}

const char* vapx_last_error(vapx_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void vapx_destroy(vapx_handle h) {
  if (!h) return;
  if (h->trunk) {
    auto& fl = h->trunk->followers;
    for (size_t i = 0; i < fl.size(); ++i)
      if (fl[i] == h) { fl.erase(fl.begin() + i); break; }
  }
  for (vapx_engine* f : h->followers) { f->trunk = nullptr; f->orphaned = true; }
  (void)hipSetDevice(h->cfg.device_id);
  (void)hipDeviceSynchronize();
#ifdef VAPX_TRACE
  auto dump_trace = [&](unsigned long long* buf, size_t wgs, const std::string& path) {   // stamps of the last traced launch: [wgs][32] u64
    if (!buf) return;
    std::vector<unsigned long long> host(wgs * 32);
    if (!host.empty() && hipMemcpy(host.data(), buf, host.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
    }
    dfree(buf);
  };
  dump_trace(h->ffn_trace, h->ffn_trace_wgs, h->ffn_trace_path);
  dump_trace(h->attn_trace, h->attn_trace_wgs, h->attn_trace_path);
#endif
  for (void* p : {(void*)h->w, (void*)h->ring, (void*)h->ring_qkv, (void*)h->h_state, (void*)h->c_state, (void*)h->carry, (void*)h->frames_seen}) dfree(p);
  release_scratch(h->sc, /*encoder_only=*/false);
  for (Staged<float>* s : {&h->audio, &h->out, &h->gw, &h->sio}) s->release();
  for (Staged<int>* s : {&h->ids, &h->mix, &h->sio_ids, &h->cls_slots}) s->release();
  for (void* p : {(void*)h->rs_hist, (void*)h->rs_out, (void*)h->rs_started, (void*)h->acc, (void*)h->mixA, (void*)h->out_c}) dfree(p);
  if (h->gstart) (void)hipEventDestroy(h->gstart);
  for (int g = 0; g < vapx_engine::kMaxGroups; ++g) {
    if (h->gdone[g]) (void)hipEventDestroy(h->gdone[g]);
    if (h->gstream[g]) (void)hipStreamDestroy(h->gstream[g]);
  }
  for (auto& r : h->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : h->prof_pool) (void)hipEventDestroy(e);
  delete h;
}

int vapx_create(const vapx_config* cfg, const float* blob, size_t n_floats, vapx_handle* out) {
  if (!cfg || !blob || !out) return fail(nullptr, VAPX_E_INVAL, "null argument");
  if (cfg->struct_size != (int32_t)sizeof(vapx_config)) return fail(nullptr, VAPX_E_INVAL, "vapx_config.struct_size mismatch");
  if (!rate_ok(cfg->frame_hz)) return fail(nullptr, VAPX_E_INVAL, "frame_hz must be 5, 10, 20 or 50");
  if (cfg->ctx_frames < 1 || cfg->ctx_frames > 512) return fail(nullptr, VAPX_E_INVAL, "ctx_frames must be in [1,512]");
  if (cfg->max_streams < 1 || cfg->max_batch < 1 || cfg->max_batch > cfg->max_streams)
    return fail(nullptr, VAPX_E_INVAL, "need 1 <= max_batch <= max_streams");
  if (cfg->mode < 0 || cfg->mode > 2) return fail(nullptr, VAPX_E_INVAL, "bad mode");
  if (cfg->mode == VAPX_MODE_NOD && cfg->ctx_frames > 256)   // pbc_rows_kernel writes p_bc of window row t into logits slot t
    return fail(nullptr, VAPX_E_INVAL, "nod mode needs ctx_frames <= 256 (got %d): the output row holds 256 p_bc slots, one per window row",
                cfg->ctx_frames);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, VAPX_E_NODEVICE, "no HIP device visible");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, VAPX_E_INVAL, "device_id out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device_id) != hipSuccess) return fail(nullptr, VAPX_E_HIP, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, VAPX_E_NODEVICE, "device %d is %s; libvapx is built for gfx950 only", cfg->device_id, prop.gcnArchName);

  vapx_engine* h = new vapx_engine();
  h->cfg = *cfg;
  static_cast<Geometry&>(*h) = geometry(cfg->frame_hz, cfg->ctx_frames);
  h->lay = vapx_layout::layout_for_K(h->ncpc, &h->lay_n);
  const size_t need = vapx_blob_floats(cfg->frame_hz);
  if (n_floats != need) {
    int rc = fail(nullptr, VAPX_E_INVAL, "weights blob has %zu floats, expected %zu for %d Hz", n_floats, need, cfg->frame_hz);
    delete h;
    return rc;
  }
#define CR(expr)                                                                                   \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      int rc = fail(nullptr, _e == hipErrorOutOfMemory ? VAPX_E_NOMEM : VAPX_E_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
      (void)hipGetLastError();   /* do not leave the error for the next launch check to find */     \
      vapx_destroy(h);                                                                             \
      return rc;                                                                                   \
    }                                                                                              \
  } while (0)
  CR(hipSetDevice(cfg->device_id));
  CR(dalloc(&h->w, need, false));
  CR(hipMemcpy(h->w, blob, need * sizeof(float), hipMemcpyHostToDevice));
  // every weight pointer is resolved here, once; `missing` names the first required entry the layout does not have
  std::string missing;
  auto find = [&](const std::string& name, bool required) -> const float* {
    for (size_t i = 0; i < h->lay_n; ++i)
      if (name == h->lay[i].name) return h->w + h->lay[i].off;
    if (required && missing.empty()) missing = name;
    return nullptr;
  };
  auto req = [&](const std::string& name) { return find(name, true); };
  Weights& wt = h->wt;
  for (int i = 0; i < 5; ++i) {
    const std::string c = "conv" + std::to_string(i), n = "cn" + std::to_string(i);
    wt.conv[i] = {req(c + ".w"), i >= 1 ? req(c + ".w16") : nullptr, i >= 2 ? req(c + ".wf") : nullptr, req(c + ".b"), req(n + ".g"), req(n + ".b")};
  }
  wt.lstm_wih = req("lstm.wih"); wt.lstm_wih16 = req("lstm.wih16"); wt.lstm_whh = req("lstm.whh"); wt.lstm_b = req("lstm.b");
  wt.down_w = req("down.w"); wt.down_wf = req("down.wf"); wt.down_b = req("down.b"); wt.down_g = req("down.g"); wt.down_beta = req("down.beta");
  wt.l0_wqkv16 = req("L0.wqkv16"); wt.l3_last16 = req("L3.last16");
  wt.comb_wa = req("comb.wa"); wt.comb_wb = req("comb.wb"); wt.comb_waT = req("comb.waT"); wt.comb_wbT = req("comb.wbT");
  wt.comb_g = req("comb.g"); wt.comb_b = req("comb.b");
  wt.head_w = req("head.w"); wt.head_wT = req("head.wT"); wt.head_b = req("head.b"); wt.vad_w = req("vad.w"); wt.vad_b = req("vad.b");
  wt.aux_w = req("aux.w"); wt.aux_b = req("aux.b");
  for (int l = 0; l < 4; ++l) {
    Layer& Lw = h->layer[l];
    // layer 0 has no cross-attention: its entries stay null there, as does wqkvp wherever the layout lacks it (tested where it is used)
    auto get = [&](const char* suffix) { return find("L" + std::to_string(l) + "." + suffix, true); };
    auto cross = [&](const char* suffix) { return find("L" + std::to_string(l) + "." + suffix, l > 0); };
    Lw.ln_self_g = get("ln_self.g"); Lw.ln_self_b = get("ln_self.b"); Lw.wqkv = get("wqkv"); Lw.wproj = get("wproj");
    Lw.ln_src_g = cross("ln_src.g"); Lw.ln_src_b = cross("ln_src.b"); Lw.wq_x = cross("wq_x"); Lw.wkv_x = cross("wkv_x");
    Lw.wproj_x = cross("wproj_x"); Lw.ln_ffn_g = get("ln_ffn.g"); Lw.ln_ffn_b = get("ln_ffn.b"); Lw.w0 = get("w0"); Lw.w3 = get("w3");
    Lw.w0f = get("w0f"); Lw.w3f = get("w3f"); Lw.wqkvf = get("wqkvf"); Lw.wkvxf = cross("wkvxf");
    Lw.wprojf = get("wprojf"); Lw.wqxf = cross("wqxf"); Lw.wprojxf = cross("wprojxf");
    Lw.w0h = get("w0h"); Lw.w3h = get("w3h"); Lw.wqkvh = get("wqkvh"); Lw.wkvxh = cross("wkvxh");
    Lw.wprojh = get("wprojh"); Lw.wqxh = cross("wqxh"); Lw.wprojxh = cross("wprojxh");
    Lw.wproj8 = get("wproj8"); Lw.wqx8 = cross("wqx8"); Lw.wprojx8 = cross("wprojx8");
    Lw.wqkvp = find("L" + std::to_string(l) + ".wqkvp", false);
  }
  if (!missing.empty()) {
    int rc = fail(nullptr, VAPX_E_INVAL, "the weights layout for %d Hz has no entry \"%s\"", cfg->frame_hz, missing.c_str());
    vapx_destroy(h);
    return rc;
  }
  if (cfg->flags & VAPX_FLAG_SPLIT_F16) {
    // Static guarantees of the split-precision path, from the weights alone (host copy of the blob):
    //  * every weight w satisfies |2^8 w| < 65504 (its f16 hi part is finite);
    //  * the GELU hidden row h = LN_ffn(x) . W0^T obeys |h_j| <= sum_k |W0[j][k]| (16 |gamma_k| + |beta_k|) because a LayerNorm output is
    //    bounded by 16 |gamma| + |beta|: a layer whose bound reaches 2^15 gets a power-of-two down-scale of the hidden operand.
    // every weight that reaches the split-precision GEMM (gemm(): conv1-4, LSTM input projection, downsample, Combinator) is stored /
    // converted as 2^8 w in f16 as well
    for (const char* nm : {"conv1.w", "conv2.w", "conv3.w", "conv4.w", "lstm.wih", "down.w", "comb.wa", "comb.wb"})
      for (size_t i = 0; i < h->lay_n; ++i)
        if (!strcmp(h->lay[i].name, nm))
          for (size_t k = 0; k < h->lay[i].n; ++k)
            if (!(fabsf(blob[h->lay[i].off + k]) < 255.0f)) {
              int rc = fail(nullptr, VAPX_E_INVAL, "VAPX_FLAG_SPLIT_F16: a weight of %s has |w| >= 255 (or is not finite); use the fp32 path", nm);
              vapx_destroy(h);
              return rc;
            }
    //  * every ChannelNorm / LayerNorm whose output is an A operand converted to f16 WITHOUT a scale (gemm() with bounded_A: cn0 .. cn3 ->
    //    conv1 .. conv4, cn4 -> lstm.wih, ln_self -> wqkv, ln_src -> wq_x; the flat-row blocks: ln_self, ln_src, ln_ffn) obeys
    //    16 |gamma_k| + |beta_k| < 65504 in every channel k (a normalised row of 256 values has |xhat| <= sqrt(255) < 16)
    {
      auto entry = [&](const std::string& name) -> const vapx_layout::Entry* {
        for (size_t i = 0; i < h->lay_n; ++i)
          if (name == h->lay[i].name) return &h->lay[i];
        return nullptr;
      };
      std::vector<std::string> norms;
      for (int i = 0; i < 5; ++i) norms.push_back("cn" + std::to_string(i));
      for (int l = 0; l < 4; ++l)
        for (const char* s : {".ln_self", ".ln_src", ".ln_ffn"}) norms.push_back("L" + std::to_string(l) + s);
      for (const std::string& nm : norms) {
        const auto *g = entry(nm + ".g"), *b = entry(nm + ".b");
        if (nm == "L0.ln_src") continue;   // layer 0 has no cross-attention: the only norm the layout may lack
        if (!g || !b) {
          int rc = fail(nullptr, VAPX_E_INVAL, "the weights layout for %d Hz has no entry \"%s.g\" / \"%s.b\"", cfg->frame_hz, nm.c_str(), nm.c_str());
          vapx_destroy(h);
          return rc;
        }
        for (size_t k = 0; k < g->n && k < b->n; ++k) {
          const double bound = 16.0 * fabs((double)blob[g->off + k]) + fabs((double)blob[b->off + k]);
          if (!(bound < 65504.0)) {
            int rc = fail(nullptr, VAPX_E_INVAL, "VAPX_FLAG_SPLIT_F16: the norm %s has 16 |gamma| + |beta| = %g >= 65504 (or not finite) in channel %zu: "
                          "its output is an unscaled f16 operand; use the fp32 path", nm.c_str(), bound, k);
            vapx_destroy(h);
            return rc;
          }
        }
      }
    }
    for (int l = 0; l < 4; ++l) {
      Layer& Lw = h->layer[l];
      auto host = [&](const float* dev) { return blob + (dev - h->w); };
      const struct { const float* p; size_t n; } mats[] = {{Lw.w0, 768 * 256}, {Lw.w3, 256 * 768}, {Lw.wqkv, 768 * 256}, {Lw.wproj, 65536},
                                                          {Lw.wq_x, 65536}, {Lw.wkv_x, 512 * 256}, {Lw.wproj_x, 65536}};
      for (const auto& m : mats) {
        if (!m.p) continue;
        const float* q = host(m.p);
        for (size_t i = 0; i < m.n; ++i)
          if (!(fabsf(q[i]) < 255.0f)) {
            int rc = fail(nullptr, VAPX_E_INVAL, "VAPX_FLAG_SPLIT_F16: a transformer weight of layer %d has |w| >= 255 (or is not finite); use the fp32 path", l);
            vapx_destroy(h);
            return rc;
          }
      }
      const float *w0 = host(Lw.w0), *gm = host(Lw.ln_ffn_g), *bt = host(Lw.ln_ffn_b);
      double worst = 0.0;
      for (int j = 0; j < 768; ++j) {
        double b = 0.0;
        for (int k = 0; k < 256; ++k) b += fabs((double)w0[j * 256 + k]) * (16.0 * fabs((double)gm[k]) + fabs((double)bt[k]));
        worst = std::max(worst, b);
      }
      float hs = 1.0f;
      while ((double)hs * worst >= 32768.0 && hs > 1e-30f) hs *= 0.5f;
      Lw.hid_scale = hs;
    }
  }
  const size_t S = cfg->max_streams, B = cfg->max_batch, T = h->T;
  CR(dalloc(&h->ring, S * 2 * T * 256));
  CR(dalloc(&h->ring_qkv, S * 2 * T * 768));   // layer-0 Q|K|V cache, one entry per ring row
  CR(dalloc(&h->h_state, S * 2 * 256));
  CR(dalloc(&h->c_state, S * 2 * 256));
  CR(dalloc(&h->carry, S * 2 * VAPX_PAD));
  CR(dalloc(&h->frames_seen, S));
  CR(h->audio.reserve(B * 2 * h->L, true));
  CR(h->ids.reserve(B, true));
  CR(h->sio_ids.reserve(S, true));
  CR(h->out.reserve_pinned(B * VAPX_OUT_STRIDE));
  for (const ScratchRow& r : kScratchTable) {   // zero-filled: the guard rows of h0 .. h3 stay zero forever
    const ScratchSlot p = r.slot(h->sc);
    if (p.f) CR(dalloc(p.f, B * r.per_slot(*h)));
    else CR(dalloc(p.i, B * r.per_slot(*h)));
  }
  h->id_stamp.assign(S, 0u);
  h->ring_direct = ring_direct_for(cfg->flags, h->T);
  h->prune_last = prune_last_for(cfg->flags, cfg->mode);
  h->force_xl = getenv("VAPX_FORCE_ATTENTION_XL") != nullptr;
  if (getenv("VAPX_POISON_SCRATCH")) {
    CR(hipMemset(h->ring, 0xFF, S * 2 * T * 256 * sizeof(float)));          // rows beyond frames_seen are never read: prove it
    CR(hipMemset(h->ring_qkv, 0xFF, S * 2 * T * 768 * sizeof(float)));
    h->poison = true;
  }
#ifdef VAPX_TRACE
  if (const char* ev = getenv("VAPX_FFN_TRACE")) {
    h->ffn_trace_path = ev;
    CR(dalloc(&h->ffn_trace, (size_t)16384 * 32));
  }
  if (const char* ev = getenv("VAPX_ATTN_TRACE")) {
    h->attn_trace_path = ev;
    CR(dalloc(&h->attn_trace, (size_t)16384 * 32));
  }
#endif
  h->n_groups = cfg->flags & 0xF;
  if (h->n_groups == 0) h->n_groups = 1;   // measured: no gain at 256 streams, +2 % at 4096 with 2
  if (h->n_groups > vapx_engine::kMaxGroups) h->n_groups = vapx_engine::kMaxGroups;
  for (int g = 0; g < h->n_groups; ++g) {
    CR(hipStreamCreateWithFlags(&h->gstream[g], hipStreamNonBlocking));
    CR(hipEventCreateWithFlags(&h->gdone[g], hipEventDisableTiming));
  }
  CR(hipEventCreateWithFlags(&h->gstart, hipEventDisableTiming));
  CR(h->sio.reserve_pinned(0));   // its event, before the synchronisation below: the blocks come with the first host-buffer state call
  CR(hipDeviceSynchronize());
#undef CR
  *out = h;
  return VAPX_OK;
}

// what a step's audio block must be, by the engine's input: the rules of include/vapx.h "Input rate", "Input format" and "Input classes"
static int check_audio(vapx_engine* h, const int32_t* stream_ids, const void* audio, int spc, int flags) {
  if (h->cls_table) {
    if (spc != 0)
      return fail(h, VAPX_E_INVAL, "samples_per_ch must be 0 on an engine with input classes: every slot's size is its stream's class's "
                  "(vapx_input_slot_bytes); a full frame with the caller's carry is defined at 16 kHz fp32 only");
    if (stream_ids && (flags & VAPX_IDS_DEVICE))
      return fail(h, VAPX_E_INVAL, "an engine with input classes needs host stream ids (VAPX_IDS_DEVICE is refused): the host computes every "
                  "slot's offset in the packed block from its stream's class");
    if ((uintptr_t)audio & 15) return fail(h, VAPX_E_INVAL, "the packed audio block of an engine with input classes must be 16-byte aligned");
  } else if (h->in_hz()) {
    if (spc != h->hop_in())
      return fail(h, VAPX_E_INVAL, "samples_per_ch must be %d (the hop at the engine's input rate of %d Hz); a full frame with the caller's carry "
                  "is defined at 16 kHz only", h->hop_in(), h->in_hz());
  } else if (spc != h->hop && spc != h->L) return fail(h, VAPX_E_INVAL, "samples_per_ch must be %d (hop) or %d (full frame)", h->hop, h->L);
  if (h->in_fmt()) {   // lane i of the input kernel reads the dword at base + 4 i
    const size_t bps = (size_t)pcm_bytes_per_sample(h->in_fmt());
    if ((uintptr_t)audio & 3) return fail(h, VAPX_E_INVAL, "audio in a raw input format must be 4-byte aligned");
    if (((size_t)spc * bps) & 3) return fail(h, VAPX_E_INVAL, "samples_per_ch = %d: a row of %zu-byte samples is not a whole number of dwords", spc, bps);
  }
  return VAPX_OK;
}

// ---- vapx_step in pieces, each straight-line for the role it serves: the leader (or a stand-alone engine), a follower at the leader's
// rate, a follower at 1/R of it ------------------------------------------------------------------------------------------------------

// overlap groups of a tick on n_run rows: streams are independent, and a second group's kernels fill the prologue / epilogue / tail bubbles
// of the first group's kernels; a group keeps at least 32 rows
static int overlap_groups(const vapx_engine* h, int n_run) {
  int G = h->n_groups;
  while (G > 1 && n_run / G < 32) --G;
  return G;
}

// May the previous tick's un-joined groups keep running under this one?  Only if this one defers too and splits the batch the same way (a
// different split re-slices the shared scratch); the leader adds: and no reset is queued (it touches state a running group may still use)
static bool same_split(const vapx_engine* h, int n, int G, bool defer_join) {
  return defer_join && n == h->pass.entries && G == h->pass.groups && !h->poison;
}

// VAPX_POISON_SCRATCH: refill what the table marks (a follower's released encoder scratch is null) and the input kernel's rows
static int poison_scratch(vapx_engine* h, hipStream_t st) {
  for (const ScratchRow& r : kScratchTable)
    if (r.poison && scratch_ptr(r, h->sc))
      HIPCHK(h, hipMemsetAsync(scratch_ptr(r, h->sc), 0xFF, (size_t)h->cfg.max_batch * r.per_slot(*h) * sizeof(float), st));
  if (h->n_cls) HIPCHK(h, hipMemsetAsync(h->rs_out, 0xFF, (size_t)h->cfg.max_batch * 2 * h->rs_row * sizeof(float), st));
  return VAPX_OK;
}

// a follower's admission: it consumes the encoder output of its leader's latest step, once
static int admit_follower(vapx_engine* h, int n, const float* audio) {
  const vapx_engine* lead = h->trunk;
  if (audio) return fail(h, VAPX_E_INVAL, "a trunk follower takes no audio (pass NULL): it consumes its leader's encoder output");
  if (lead->tick == 0 || lead->tick == h->followed_tick)
    return fail(h, VAPX_E_INVAL, "step the trunk leader first: no new encoder output since this follower's last step");
  if (n != lead->pass.entries) return fail(h, VAPX_E_INVAL, "n=%d differs from the leader's latest step (%d streams)", n, lead->pass.entries);
  if (h->R > 1 && !lead->last_ids_known)
    return fail(h, VAPX_E_INVAL, "the leader's latest step took device stream ids (VAPX_IDS_DEVICE): a follower at 1/%d of the leader's rate "
                "needs host ids (or none), the host decides which streams have a frame due", h->R);
  return VAPX_OK;
}

// A slower follower's due-plan.  The host advances every stream's phase and sorts the batch into due entries (compact slots 0 .. n_due-1 of
// this engine's chain) and collecting ones; trunk_collect_kernel does the rest, keyed by stream id.  The plan stays in h->mix.dev as
// [stream id | leader slot | pos][n]: its first n_due ids are the due streams', in compact order
static int count_due(const vapx_engine* h, int n) {
  const int32_t* lid = h->trunk->last_ids_host.data();
  int n_due = 0;
  for (int i = 0; i < n; ++i) n_due += h->phase[lid[i]] + 1 == h->R;
  return n_due;
}
static int plan_due(vapx_engine* h, int n, int n_due, hipStream_t st) {
  const vapx_engine* lead = h->trunk;
  if (lead->deferred_pending)   // the collect reads every overlap group's LSTM rows (the leader's own flag stays: only `st` waits)
    for (int g = 0; g < lead->pass.groups; ++g) HIPCHK(h, hipStreamWaitEvent(st, lead->gdone[g], 0));
  const int32_t* lid = lead->last_ids_host.data();
  int *e_sid = h->mix_host.data(), *e_slot = e_sid + n, *e_pos = e_sid + 2 * n;
  int kd = 0, kn = n_due;
  for (int i = 0; i < n; ++i) {
    const int sid = lid[i], ph = h->phase[sid];
    const bool due = ph + 1 == h->R;
    const int k = due ? kd++ : kn++;
    e_sid[k] = sid; e_slot[k] = i; e_pos[k] = ph;
    h->phase[sid] = due ? 0 : ph + 1;
  }
  HIPCHK(h, h->mix.upload(e_sid, (size_t)3 * n, st));
  TrunkCollectArgs ca;
  ca.lstm_out = lead->sc.lstm_out; ca.acc = h->acc; ca.A = h->mixA; ca.sid = h->mix.dev; ca.slot = h->mix.dev + n; ca.pos = h->mix.dev + 2 * n;
  ca.frames_seen = h->frames_seen; ca.bn = h->sc.bn; ca.bhead = h->sc.bhead;
  ca.n = n; ca.n_due = n_due; ca.ncpc_l = lead->ncpc; ca.R = h->R; ca.T = h->T;
  ProfScope ps(h, CLS_TRUNK_COLLECT, st);
  HIPCHK(h, launch_trunk_collect(ca, st));
  return VAPX_OK;
}

// The leader's input of one batch, on `st`: the caller's block - [n][2][spc] samples of the engine's format, or a table's packed slots,
// whose descriptors the host builds - goes to the device (unless it is there) and, on an engine with input classes, through ONE launch of
// the input kernel.  What conv0 and its carry see afterwards is plain rows: [n][2][spc] fp32 at 16 kHz.  Nothing here knows of a step
struct InputRows { const float* rows; int spc; };
static int stage_input(vapx_engine* h, int n, const int32_t* stream_ids, const int* ids_dev, const float* audio, int spc, int flags,
                       hipStream_t st, InputRows* out) {
  size_t bytes = (size_t)n * 2 * spc * (size_t)pcm_bytes_per_sample(h->in_fmt());
  if (h->cls_table) {
    bytes = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t* c = &h->stream_cls[(size_t)2 * (stream_ids ? stream_ids[i] : i)];
      h->cls_slots_host[i] = {(uint32_t)bytes, input_slot_classes(c[0], c[1])};
      // channel 1's row, then channel 2's.  Below 2^32: vapx_set_input_classes refused a table whose largest same-class slot x max_batch
      // is not, and row(c1) + row(c2) <= 2 max(row) = the largest same-class slot
      bytes += h->cls_row_bytes(c[0]) + h->cls_row_bytes(c[1]);
    }
    HIPCHK(h, h->cls_slots.upload((const int*)h->cls_slots_host.data(), (size_t)2 * n, st));
  }
  const float* ad = audio;
  if (!(flags & VAPX_AUDIO_DEVICE)) {
    // pageable memory: stage through the engine's pinned buffer (an async copy from pageable memory is a hidden synchronous staging
    // copy inside the runtime); vapx_host_alloc memory: copy straight from the caller.  `bytes` is a whole number of dwords
    // (check_audio; a table's slots are multiples of 16) and never more than `audio` holds (build_input)
    HIPCHK(h, h->audio.upload(audio, bytes / sizeof(float), st, is_pinned_host(audio)));
    ad = h->audio.dev;
  }
  if (h->n_cls) {   // the block -> 16 kHz fp32 rows, one launch for the whole batch before the overlap groups fork
    if (h->rs_row == h->hop) spc = h->hop;   // else a uniform 16 kHz engine: hop or full frame, as stepped
    InputClassesArgs ia;
    ia.in = (const unsigned char*)ad; ia.slots = h->cls_table ? (const InputSlot*)h->cls_slots.dev : nullptr; ia.ids = ids_dev;
    ia.hist = h->rs_hist; ia.started = h->rs_started; ia.out = h->rs_out; ia.rec = h->rs_rec; ia.out_row = spc;
    memcpy(ia.cls, h->cls, sizeof ia.cls);
    HIPCHK(h, launch_input_classes(ia, n, h->cls_lds, st));
    ad = h->rs_out;
  }
  *out = {ad, spc};
  return VAPX_OK;
}

// where a group's encoder output comes from: the engine's own encoder on `audio` (rows of `spc` samples), or - a follower - LSTM rows
// that exist already in `trunk`, a Scratch sliced by `trunk_geo`
struct GroupFeed { const float* audio; int spc; const Scratch* trunk; const Geometry* trunk_geo; };

// fork, run, join: the tick's rows [0, n_run) in G groups on HIP streams of their own (G = 1: on `st` itself); with defer_join the groups
// are left running and `st` does not wait
static int run_groups(vapx_engine* h, int n_run, int G, const int* ids, const GroupFeed& in, float* orows, hipStream_t st, bool defer_join) {
  if (G > 1) {
    HIPCHK(h, hipEventRecord(h->gstart, st));
    for (int g = 0; g < G; ++g) HIPCHK(h, hipStreamWaitEvent(h->gstream[g], h->gstart, 0));
  }
  for (int g = 0; g < G && n_run > 0; ++g) {
    const int b0 = (int)((long)n_run * g / G), nb = (int)((long)n_run * (g + 1) / G) - b0;
    hipStream_t gs = G > 1 ? h->gstream[g] : st;
    Scratch trunk;
    if (in.trunk) trunk = in.trunk->slice(b0, *in.trunk_geo);
    const int rc = step_group(h, h->sc.slice(b0, *h), nb, b0, ids ? ids + b0 : nullptr, in.audio ? in.audio + (size_t)b0 * 2 * in.spc : nullptr,
                              in.spc, orows + (size_t)b0 * VAPX_OUT_STRIDE, gs, in.trunk ? &trunk : nullptr);
    if (rc) return rc;
    if (G > 1) HIPCHK(h, hipEventRecord(h->gdone[g], gs));
  }
  if (G > 1 && !defer_join)
    for (int g = 0; g < G; ++g) HIPCHK(h, hipStreamWaitEvent(st, h->gdone[g], 0));
  return VAPX_OK;
}

// The end of a host-output call.  With `from`: its device block (or `src`) first travels to `rows`, the caller's memory (vapx_host_alloc
// memory: the copy lands there directly), and `st` is synchronised.  Then e->bad_slots lists the rows - n of them, `stride` floats apart -
// that carry VAPX_OUT_STATUS = 1, non-finite results (VAPX_STATUS_NO_FRAME, 2, is no fault)
static int finish_host_rows(vapx_engine* e, Staged<float>* from, const float* src, size_t bytes, float* rows, int n, size_t stride, hipStream_t st) {
  if (from) {
    HIPCHK(e, from->download(rows, bytes, st, src));
    HIPCHK(e, hipStreamSynchronize(st));
  }
  e->bad_slots.clear();
  for (int i = 0; i < n; ++i)
    if (rows[(size_t)i * stride + VAPX_OUT_STATUS] == 1.f) e->bad_slots.push_back(i);
  return VAPX_OK;
}

// the tick is enqueued: what the next call, vapx_peek and vapx_join find; then the output rows of a host-output step
static int finish_step(vapx_engine* h, int n, int G, const int* ids, bool defer_join, const int32_t* host_ids, float* out, int flags, hipStream_t st) {
  h->deferred_pending = defer_join;
  h->pass.groups = G; h->pass.entries = n; h->pass.prefill = false;
  h->last_ids = ids;
  if (h->trunk) h->followed_tick = h->trunk->tick; else ++h->tick;
  if (flags & VAPX_OUT_DEVICE) return VAPX_OK;
  const int rc = finish_host_rows(h, &h->out, h->sc.out_dev, (size_t)n * VAPX_OUT_STRIDE * sizeof(float), out, n, VAPX_OUT_STRIDE, st);
  if (rc || h->bad_slots.empty()) return rc;
  // Fail loudly rather than hand NaNs to a dialogue system — but per stream: the out block is complete, the healthy rows
  // are valid, the offending batch slots carry VAPX_OUT_STATUS = 1 and are listed by vapx_bad_slots().
  const int i = h->bad_slots[0];
  return fail(h, VAPX_E_NUMERIC, "non-finite outputs for batch slot %d (stream %d) and %zu more; the other rows are valid; these streams' state is "
              "poisoned: reset them (vapx_bad_slots lists the slots)", i, host_ids ? host_ids[i] : i, h->bad_slots.size() - 1);
}

static int step_leader(vapx_engine* h, int n, const int32_t* stream_ids, const float* audio, int spc, float* out, int flags, hipStream_t st) {
  const int32_t* host_ids = stream_ids && !(flags & VAPX_IDS_DEVICE) ? stream_ids : nullptr;
  if (!audio) return fail(h, VAPX_E_INVAL, "null audio");
  int rc = check_audio(h, stream_ids, audio, spc, flags);
  if (rc || (host_ids && (rc = check_ids(h, n, host_ids))) || (rc = enter(h))) return rc;
  const int G = overlap_groups(h, n);
  // free-running groups are only safe when nothing of this step is staged through engine-owned buffers on `st` (host audio / host ids
  // would be overwritten under a still-running group of the previous tick); rs_out is one buffer: the next tick's input launch must not
  // overtake a running group
  const bool defer_join = G > 1 && (flags & VAPX_DEFER_JOIN) && (flags & VAPX_OUT_DEVICE) && (flags & VAPX_AUDIO_DEVICE) && !host_ids && !h->n_cls;
  if (!(same_split(h, n, G, defer_join) && h->pending_resets.empty()) && (rc = settle(h, st))) return rc;   // the fast path: nothing is joined
  if (h->poison && (rc = poison_scratch(h, st))) return rc;
  const int* ids = nullptr;
  if ((rc = upload_ids(h, h->ids, n, stream_ids, flags, st, &ids))) return rc;
  h->last_ids_known = !(stream_ids && (flags & VAPX_IDS_DEVICE));   // what a slower follower walks: this step's stream ids on the host
  if (h->last_ids_known && !h->followers.empty()) {
    h->last_ids_host.resize(n);
    for (int i = 0; i < n; ++i) h->last_ids_host[i] = stream_ids ? stream_ids[i] : i;
  }
  InputRows in;
  if ((rc = stage_input(h, n, stream_ids, ids, audio, spc, flags, st, &in))) return rc;
  h->pass.tail_fused = false;   // run_conv_chain sets it per group
  rc = run_groups(h, n, G, ids, GroupFeed{in.rows, in.spc, nullptr, nullptr}, (flags & VAPX_OUT_DEVICE) ? out : h->sc.out_dev, st, defer_join);
  return rc ? rc : finish_step(h, n, G, ids, defer_join, host_ids, out, flags, st);
}

// a follower at its leader's rate: the same streams in the same order as the leader's step, the leader's LSTM rows group by group
static int step_same_rate(vapx_engine* h, int n, const int32_t* host_ids, float* out, int flags, hipStream_t st) {
  const vapx_engine* lead = h->trunk;
  const int G = overlap_groups(h, n);
  const bool defer_join = G > 1 && (flags & VAPX_DEFER_JOIN) && (flags & VAPX_OUT_DEVICE) && !host_ids;
  int rc = VAPX_OK;
  if (!same_split(h, n, G, defer_join) && (rc = join_deferred(h, st))) return rc;
  if (h->poison && (rc = poison_scratch(h, st))) return rc;
  rc = run_groups(h, n, G, lead->last_ids, GroupFeed{nullptr, 0, &lead->sc, lead}, (flags & VAPX_OUT_DEVICE) ? out : h->sc.out_dev, st, defer_join);
  return rc ? rc : finish_step(h, n, G, lead->last_ids, defer_join, host_ids, out, flags, st);
}

// a follower at 1/R of its leader's rate: its chain runs on the streams with a frame due this tick, compact; one scatter places their rows
// (and the others' VAPX_STATUS_NO_FRAME rows) in the caller's block.  It never defers: its groups split the due streams
static int step_slower(vapx_engine* h, int n, const int32_t* host_ids, float* out, int flags, hipStream_t st) {
  const int n_due = count_due(h, n), G = overlap_groups(h, n_due);
  int rc = VAPX_OK;
  if ((h->poison && (rc = poison_scratch(h, st))) || (rc = plan_due(h, n, n_due, st))) return rc;
  Scratch collected;   // the collected operand: this engine's own n_cpc rows per frame
  collected.lstm_out = h->mixA;
  if ((rc = run_groups(h, n_due, G, h->mix.dev, GroupFeed{nullptr, 0, &collected, h}, h->out_c, st, false))) return rc;
  {
    OutScatterArgs oa{h->out_c, (flags & VAPX_OUT_DEVICE) ? out : h->sc.out_dev, h->mix.dev + n, n, n_due, VAPX_OUT_STRIDE};
    ProfScope ps(h, CLS_TRUNK_COLLECT, st);
    HIPCHK(h, launch_out_scatter(oa, st));
  }
  return finish_step(h, n, G, h->mix.dev, false, host_ids, out, flags, st);
}

int vapx_step(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* audio, int32_t spc, float* out,
              int32_t flags, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  if (n < 1 || n > h->cfg.max_batch) return fail(h, VAPX_E_RANGE, "n=%d outside [1,%d]", n, h->cfg.max_batch);
  if (!out) return fail(h, VAPX_E_INVAL, "null out");
  if (h->orphaned) return fail(h, VAPX_E_INVAL, "the trunk leader of this engine was destroyed");
  if (!stream_ids && n > h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "n exceeds max_streams");
  hipStream_t st = (hipStream_t)hip_stream;
  if (!h->trunk) return step_leader(h, n, stream_ids, audio, spc, out, flags, st);
  const int32_t* host_ids = stream_ids && !(flags & VAPX_IDS_DEVICE) ? stream_ids : nullptr;   // ignored, but for what may be deferred
  int rc = admit_follower(h, n, audio);
  if (rc || (rc = enter(h))) return rc;
  return h->R > 1 ? step_slower(h, n, host_ids, out, flags, st) : step_same_rate(h, n, host_ids, out, flags, st);
}

int32_t vapx_bad_slots(vapx_handle h, int32_t* slots, int32_t max_slots) {
  if (!h) return VAPX_E_INVAL;
  const int32_t n = (int32_t)h->bad_slots.size();
  for (int32_t i = 0; i < n && i < max_slots && slots; ++i) slots[i] = h->bad_slots[i];
  return n;
}

size_t vapx_group_wire_floats(vapx_handle h) {
  if (!h || h->trunk || h->orphaned) return 0;
  size_t per = (size_t)vapx_wire_floats(h->cfg.mode, h->T);
  for (vapx_engine* f : h->followers) per += (size_t)vapx_wire_floats(f->cfg.mode, f->T);
  return per;
}

int vapx_step_group(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* audio, int32_t spc, float* wire_out,
                    int32_t flags, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  if (h->trunk || h->orphaned) return fail(h, VAPX_E_INVAL, "vapx_step_group takes the trunk leader; this engine is a follower");
  if (n < 1 || n > h->cfg.max_batch) return fail(h, VAPX_E_RANGE, "n=%d outside [1,%d]", n, h->cfg.max_batch);
  if (!wire_out) return fail(h, VAPX_E_INVAL, "null wire_out");
  for (size_t i = 0; i < h->followers.size(); ++i)
    if (h->followers[i]->followed_tick != h->tick)
      return fail(h, VAPX_E_INVAL, "follower %zu has not consumed the leader's latest vapx_step yet: step it first (or step the whole group "
                  "with vapx_step_group every tick)", i);
  hipStream_t st = (hipStream_t)hip_stream;
  const bool to_host = !(flags & VAPX_OUT_DEVICE);
  const size_t per = vapx_group_wire_floats(h);
  if (int rc = enter(h)) return rc;
  if (to_host) HIPCHK(h, h->gw.reserve(per * (size_t)h->cfg.max_batch, true));
  // every model device-resident, on the one stream: exactly the vapx_step(.., VAPX_OUT_DEVICE, ..) path (VAPX_DEFER_JOIN is dropped:
  // the pack kernel below consumes every overlap group's rows)
  int rc = vapx_step(h, n, stream_ids, audio, spc, h->sc.out_dev, (flags & (VAPX_AUDIO_DEVICE | VAPX_IDS_DEVICE)) | VAPX_OUT_DEVICE, hip_stream);
  if (rc) return rc;
  for (size_t i = 0; i < h->followers.size(); ++i) {
    vapx_engine* f = h->followers[i];
    rc = vapx_step(f, n, nullptr, nullptr, 0, f->sc.out_dev, VAPX_OUT_DEVICE, hip_stream);
    if (rc) return fail(h, rc, "follower %zu: %s", i, f->err.c_str());
  }
  float* wd = to_host ? h->gw.dev : wire_out;
  const int M = 1 + (int)h->followers.size();
  std::vector<int> wf(M);
  std::vector<size_t> off(M);
  size_t acc = 0;
  for (int m = 0; m < M; ++m) {
    const vapx_engine* e = m ? h->followers[m - 1] : h;
    wf[m] = vapx_wire_floats(e->cfg.mode, e->T);
    off[m] = (size_t)n * acc;
    acc += (size_t)wf[m];
  }
  for (int m0 = 0; m0 < M; m0 += 4) {   // one launch for up to four models
    WirePackArgs a;
    memset(&a, 0, sizeof a);
    a.dst = wd; a.n = n; a.src_stride = VAPX_OUT_STRIDE; a.n_models = std::min(4, M - m0);
    for (int k = 0; k < a.n_models; ++k) {
      a.src[k] = (m0 + k) ? h->followers[m0 + k - 1]->sc.out_dev : h->sc.out_dev;
      a.dst_off[k] = (long)off[m0 + k];
      a.wf4[k] = wf[m0 + k] / 4;
    }
    HIPCHK(h, launch_wire_pack(a, st));
  }
  h->group_bad.clear();
  if (!to_host) return VAPX_OK;
  // per stream and per model, as vapx_step: the block is complete, the offending rows carry VAPX_OUT_STATUS = 1.  The leader's call
  // brings the whole block: the one D2H copy of the tick
  for (int m = 0; m < M; ++m) {
    vapx_engine* e = m ? h->followers[m - 1] : h;
    rc = finish_host_rows(e, m ? nullptr : &h->gw, nullptr, (size_t)n * per * sizeof(float), wire_out + off[m], n, (size_t)wf[m], st);
    if (rc) return rc;
    for (int i : e->bad_slots) h->group_bad.push_back({i, m});
  }
  if (!h->group_bad.empty())
    return fail(h, VAPX_E_NUMERIC, "non-finite outputs for batch slot %d in model %d and %zu more (slot, model) pairs; the other rows are valid; "
                "reset those streams on the leader (vapx_group_bad lists the pairs)", h->group_bad[0].first, h->group_bad[0].second,
                h->group_bad.size() - 1);
  return VAPX_OK;
}

int32_t vapx_group_bad(vapx_handle h, int32_t* slots, int32_t* models, int32_t max) {
  if (!h) return VAPX_E_INVAL;
  const int32_t n = (int32_t)h->group_bad.size();
  for (int32_t i = 0; i < n && i < max; ++i) {
    if (slots) slots[i] = h->group_bad[i].first;
    if (models) models[i] = h->group_bad[i].second;
  }
  return n;
}

void* vapx_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void vapx_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int vapx_join(vapx_handle h, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  if (int rc = enter(h)) return rc;
  for (int g = 0; g < h->pass.groups && h->pass.groups > 1; ++g) HIPCHK(h, hipStreamWaitEvent((hipStream_t)hip_stream, h->gdone[g], 0));
  return VAPX_OK;   // deferred_pending stays set: only `hip_stream` waited, a later step on another stream still has to
}

int vapx_attach_trunk(vapx_handle f, vapx_handle lead) {
  if (!f || !lead) return VAPX_E_INVAL;
  if (f == lead || lead->trunk || f->trunk || !f->followers.empty())
    return fail(f, VAPX_E_INVAL, "attach a stand-alone engine to a leader that is not itself a follower");
  if (f->tick != 0 || lead->tick != 0) return fail(f, VAPX_E_INVAL, "attach before the first step of either engine");
  if (f->n_cls) {
    if (f->in_hz()) return fail(f, VAPX_E_INVAL, "this engine has an input rate of its own (%d Hz): a follower takes no audio, set the rate on the leader", f->in_hz());
    if (f->cls_table) return fail(f, VAPX_E_INVAL, "this engine has input classes of its own: a follower takes no audio, set the table on the leader");
    return fail(f, VAPX_E_INVAL, "this engine has an input format of its own (%d): a follower takes no audio, set the format on the leader", f->in_fmt());
  }
  if (f->cfg.device_id != lead->cfg.device_id || f->cfg.max_streams != lead->cfg.max_streams || f->cfg.max_batch != lead->cfg.max_batch)
    return fail(f, VAPX_E_INVAL, "device, max_streams and max_batch must match the leader's");
  // window and rate may differ: the follower's frame is R consecutive leader ticks (a CPC frame is a function of real samples only)
  if (lead->cfg.frame_hz < f->cfg.frame_hz)
    return fail(f, VAPX_E_INVAL, "the leader (%d Hz) is slower than this follower (%d Hz): the group's fastest model leads, a follower "
                "cannot make frames its leader never encodes", lead->cfg.frame_hz, f->cfg.frame_hz);
  if (lead->cfg.frame_hz % f->cfg.frame_hz != 0)
    return fail(f, VAPX_E_INVAL, "the leader's frame_hz (%d) is not an integer multiple of this follower's (%d): the follower's frames "
                "would not end on leader ticks", lead->cfg.frame_hz, f->cfg.frame_hz);
  const int R = lead->cfg.frame_hz / f->cfg.frame_hz;
  if (f->ncpc != R * lead->ncpc) return fail(f, VAPX_E_INVAL, "internal: n_cpc %d is not %d x the leader's %d", f->ncpc, R, lead->ncpc);
  HIPCHK(f, hipSetDevice(f->cfg.device_id));
  HIPCHK(f, hipDeviceSynchronize());
  {  // the CPC CNN + LSTM weights must be the same tensors (they come from the common cpc_model file, vap_main.py:199-201)
    const float* a0 = f->wt.conv[0].w; const float* a1 = f->wt.down_w;
    const float* b0 = lead->wt.conv[0].w;
    const size_t nfl = (size_t)(a1 - a0);
    std::vector<float> ha(nfl), hb(nfl);
    HIPCHK(f, hipMemcpy(ha.data(), a0, nfl * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(f, hipMemcpy(hb.data(), b0, nfl * sizeof(float), hipMemcpyDeviceToHost));
    if (memcmp(ha.data(), hb.data(), nfl * sizeof(float)) != 0)
      return fail(f, VAPX_E_INVAL, "CPC encoder weights differ from the leader's: nothing to share");
  }
  if (R > 1) {
    const size_t S = f->cfg.max_streams, B = f->cfg.max_batch;
    hipError_t e = dalloc(&f->acc, S * 2 * (size_t)(R - 1) * lead->ncpc * 256);
    if (e == hipSuccess) e = dalloc(&f->mixA, B * 2 * (size_t)f->ncpc * 256);
    if (e == hipSuccess) e = dalloc(&f->out_c, B * VAPX_OUT_STRIDE);
    if (e == hipSuccess) e = f->mix.reserve(3 * B, true);
    if (e != hipSuccess) {   // nothing of the engine is released yet: it stays a stand-alone engine
      (void)hipGetLastError();
      return fail(f, e == hipErrorOutOfMemory ? VAPX_E_NOMEM : VAPX_E_HIP, "state of a 1/%d-rate follower: %s", R, hipGetErrorString(e));
    }
    f->phase.assign(S, 0);
    f->mix_host.assign(3 * B, 0);
  }
  // a follower never runs the encoder: release its encoder scratch and LSTM / carry state
  release_scratch(f->sc, /*encoder_only=*/true);
  f->audio.release();
  for (float** p : {&f->h_state, &f->c_state, &f->carry}) { dfree(*p); *p = nullptr; }
  f->R = R;
  f->own_window = R == 1 && f->T != lead->T;
  f->trunk = lead;
  lead->followers.push_back(f);
  return VAPX_OK;
}

int vapx_reset_stream(vapx_handle h, int32_t sid) {
  if (!h) return VAPX_E_INVAL;
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id out of range");
  if (h->trunk) return fail(h, VAPX_E_INVAL, "reset the trunk leader: it resets its followers too");
  // No device work and no synchronisation here: the request is queued and the NEXT vapx_step applies it with one tiny
  // kernel ordered on its HIP stream, before that step touches any state — a joining client costs the other streams nothing.
  for (int32_t& q : h->pending_resets) {
    if (q == sid) return VAPX_OK;
    if (q == -sid - 1) { q = sid; return VAPX_OK; }   // a queued carry-only reset is subsumed
  }
  h->pending_resets.push_back(sid);
  return VAPX_OK;
}

int vapx_reset_carry(vapx_handle h, int32_t sid) {
  if (!h) return VAPX_E_INVAL;
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id out of range");
  if (h->trunk) return fail(h, VAPX_E_INVAL, "the carry lives in the trunk leader");
  for (int32_t q : h->pending_resets)
    if (q == sid || q == -sid - 1) return VAPX_OK;   // a full reset (or the same request) is already queued
  h->pending_resets.push_back(-sid - 1);
  return VAPX_OK;
}

int vapx_get_config(vapx_handle h, vapx_config* out) {
  if (!h || !out) return VAPX_E_INVAL;
  *out = h->cfg;
  return VAPX_OK;
}

// ---- stream state in and out: vapx_get_state / vapx_set_state and the bulk calls (vapx.h "Bulk state export / import") -----------------
// One mover: the gather / scatter kernels of state_io.hip on a record laid out by state_record.h.  The bulk calls move the public record,
// stream-ordered; the per-stream calls move one engine-internal record (no resampler history, no cache) on the null stream.
namespace {

constexpr size_t kStateStageFloats = (size_t)8 << 20;   // 32 MiB: host records travel through device / pinned blocks of at most this size

bool sio_follower(const vapx_engine* h) { return h->trunk != nullptr || h->orphaned; }

StateLayout sio_layout(const vapx_engine* h, int flags) { return state_layout(h->T, !sio_follower(h), h->rs_rec, (flags & VAPX_STATE_CACHE) != 0); }
size_t state_floats(const vapx_engine* h, int flags) { return (size_t)sio_layout(h, flags).total; }

// argument checks of the bulk calls; host ids are validated here, before anything is enqueued
int sio_check(vapx_engine* h, const char* what, int n, const int32_t* ids, const void* buf, int flags) {
  if (h->cls_table) return fail(h, VAPX_E_INVAL, "%s is refused on an engine with input classes: a state record has one resampler history size per engine, "
                            "records with per-stream history sizes do not exist yet (vapx_get_state / vapx_set_state work)", what);
  if (h->R > 1)   // the record has no place yet for the leader rows of a frame in the making (acc) and the stream's phase
    return fail(h, VAPX_E_INVAL, "%s: refused on a trunk follower at 1/%d of its leader's rate: a state record does not carry the stream's "
                "half-collected frame and phase yet (vapx_get_state / vapx_set_state move its ring)", what, h->R);
  if (n < 1 || n > h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "%s: n=%d outside [1,%d] (max_streams)", what, n, h->cfg.max_streams);
  if (!buf) return fail(h, VAPX_E_INVAL, "%s: null record buffer", what);
  if ((uintptr_t)buf & 15) return fail(h, VAPX_E_INVAL, "%s: the record buffer must be 16-byte aligned", what);
  if (flags & ~(VAPX_STATE_CACHE | VAPX_OUT_DEVICE | VAPX_IDS_DEVICE)) return fail(h, VAPX_E_INVAL, "%s: unknown flag bits 0x%x", what, flags);
  if (ids && !(flags & VAPX_IDS_DEVICE)) return check_ids(h, n, ids);
  return VAPX_OK;
}

// the staging blocks at `want` floats.  Every host-buffer call ends with the stream synchronised, so a block that has to grow is idle
int sio_reserve(vapx_engine* h, size_t want, bool need_pinned) {
  hipError_t e = h->sio.reserve(want, false);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, VAPX_E_NOMEM, "state staging block (%zu bytes, device): %s", want * 4, hipGetErrorString(e)); }
  if (need_pinned && (e = h->sio.reserve_pinned(want)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, VAPX_E_NOMEM, "state staging block (%zu bytes, pinned): %s", want * 4, hipGetErrorString(e));
  }
  return VAPX_OK;
}

// staging blocks for the bulk calls' host records: streams per block (>= 1).  (The ids of a state call, up to max_streams of them, travel
// through sio_ids: the step's id buffers hold max_batch)
int sio_stage(vapx_engine* h, size_t rec, int n, bool need_pinned, int* per_block) {
  size_t cap = kStateStageFloats;
  if (const char* ev = getenv("VAPX_STATE_STAGE_FLOATS")) {   // debug knob: small blocks, so that a test with a handful of streams takes the multi-block path
    const long v = atol(ev);
    if (v > 0) cap = (size_t)v;
  }
  size_t per = cap / rec;
  if (per < 1) per = 1;
  if (per > (size_t)n) per = (size_t)n;
  *per_block = (int)per;
  return sio_reserve(h, per * rec, need_pinned);
}

// kernel arguments for n records of layout L at `rec`, every section of the layout named; the header words say what the record holds
StateIoArgs sio_args(vapx_engine* h, const StateLayout& L, float* rec, const int* ids, int n) {
  StateIoArgs a;
  memset(&a, 0, sizeof a);
  a.rec = rec; a.lay = L; a.sections = L.sections(); a.ids = ids; a.id0 = 0;
  a.ring = h->ring; a.ring_qkv = h->ring_qkv; a.h_state = h->h_state; a.c_state = h->c_state; a.carry = h->carry;
  a.frames_seen = h->frames_seen; a.T = h->T; a.n = n;
  const bool history = L.history >= 0;   // of the bulk calls' record, on an engine with an input rate
  a.rs_hist = history ? h->rs_hist : nullptr; a.rs_started = history ? h->rs_started : nullptr; a.rs_rec = history ? h->rs_rec : 0;
  a.hdr[SH_MAGIC] = VAPX_STATE_MAGIC; a.hdr[SH_CTX_FRAMES] = h->T; a.hdr[SH_FRAME_HZ] = h->cfg.frame_hz;
  a.hdr[SH_BITS] = (L.lstm >= 0 ? VAPX_STATE_HAS_LSTM : 0) | (history ? VAPX_STATE_HAS_RESAMPLE : 0) |
                   (L.cache >= 0 ? VAPX_STATE_HAS_CACHE | ((h->cfg.flags & VAPX_FLAG_SPLIT_F16) ? VAPX_STATE_CACHE_SPLIT : 0) : 0);
  a.hdr[SH_MODE] = h->cfg.mode; a.hdr[SH_INPUT_HZ] = history ? h->in_hz() : 0;
  return a;
}

// rebuild the layer-0 Q|K|V cache of n streams (ids, or id0 + k) from their ring rows: LN(ring rows) . Wqkv^T (fp32 path), for up to
// max_batch streams per pass through the step's scratch: LN, one GEMM, one scatter of the rows below the window fill - whatever the
// number of streams in the pass
int rebuild_cache(vapx_engine* h, const int* ids, int id0, int n, hipStream_t st) {
  const int B = h->cfg.max_batch, T = h->T;
  for (int k0 = 0; k0 < n; k0 += B) {
    const int nb = std::min(B, n - k0);
    const int* cids = ids ? ids + k0 : nullptr;
    { ProfScope ps(h, CLS_GATHER, st);
      HIPCHK(h, launch_state_ln(h->ring, cids, id0 + k0, h->sc.xn, h->layer[0].ln_self_g, h->layer[0].ln_self_b, T, nb, st)); }
    GemmArgs g = gemm_args(h->sc.xn, contiguous_rows(256), h->layer[0].wqkv, nb * 2 * T, 768, 256, h->sc.qkv, contiguous_rows(768));
    { ProfScope ps(h, gemm_class(EPI_STORE), st); HIPCHK(h, launch_gemm_f32(g, EPI_STORE, 0, st)); }
    HIPCHK(h, launch_state_cache_scatter(h->sc.qkv, cids, id0 + k0, h->ring_qkv, h->frames_seen, T, nb, st));
  }
  return VAPX_OK;
}

// the per-stream calls, once their arguments are checked: the device idle, then kernel arguments for stream `sid` and an engine-internal
// record - its ring and, unless this is a follower, LSTM + carry - in the staging blocks.  Not the public format's business: no sio_check,
// no staging bound
int sio_one(vapx_engine* h, int sid, StateIoArgs* a) {
  if (int rc = quiesce(h)) return rc;
  const StateLayout L = state_layout(h->T, !sio_follower(h), 0, false);
  if (int rc = sio_reserve(h, (size_t)L.total, true)) return rc;
  *a = sio_args(h, L, h->sio.dev, nullptr, 1);
  a->id0 = sid;
  return VAPX_OK;
}

}  // namespace

int vapx_get_state(vapx_handle h, int32_t sid, float* ring, int32_t* n_frames, float* lstm, float* carry) {
  if (!h) return VAPX_E_INVAL;
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id out of range");
  if (sio_follower(h) && (lstm || carry)) return fail(h, VAPX_E_INVAL, "LSTM / carry state lives in the trunk leader");
  StateIoArgs a;
  if (int rc = sio_one(h, sid, &a)) return rc;
  const StateLayout& L = a.lay;
  HIPCHK(h, launch_state_export(a, nullptr));
  const float* r = h->sio.pin;
  HIPCHK(h, h->sio.download(h->sio.pin, (size_t)L.total * sizeof(float), nullptr));   // page-locked: one asynchronous copy
  HIPCHK(h, hipStreamSynchronize(nullptr));
  int32_t n = 0;
  memcpy(&n, r + L.header + SH_N_FRAMES, sizeof n);
  if (n_frames) *n_frames = n;
  if (ring)   // rows t < n_frames; the caller's rows beyond stay as they are
    for (int c = 0; c < 2; ++c) memcpy(ring + (size_t)c * h->T * 256, r + L.ring + (size_t)c * h->T * 256, (size_t)n * 256 * sizeof(float));
  if (lstm) memcpy(lstm, r + L.lstm, kStateLstmFloats * sizeof(float));
  if (carry) memcpy(carry, r + L.carry, kStateCarryFloats * sizeof(float));
  return VAPX_OK;
}

int vapx_set_state(vapx_handle h, int32_t sid, const float* ring, int32_t n_frames, const float* lstm, const float* carry) {
  if (!h) return VAPX_E_INVAL;
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id out of range");
  if (n_frames < 0 || n_frames > h->T) return fail(h, VAPX_E_INVAL, "n_frames outside [0,T]");
  if (sio_follower(h) && (lstm || carry)) return fail(h, VAPX_E_INVAL, "LSTM / carry state lives in the trunk leader");
  StateIoArgs a;
  if (int rc = sio_one(h, sid, &a)) return rc;
  const StateLayout& L = a.lay;
  a.sections = (ring ? SEC_RING : 0) | (lstm ? SEC_LSTM : 0) | (carry ? SEC_CARRY : 0);
  HIPCHK(h, h->sio.acquire_pinned());
  float* r = h->sio.pin;
  a.hdr[SH_N_FRAMES] = n_frames;
  memcpy(r + L.header, a.hdr, sizeof a.hdr);
  // chronological rows land in slots 0..n-1 and frames_seen = n, so the next append goes to slot n % T
  if (ring)
    for (int c = 0; c < 2; ++c) memcpy(r + L.ring + (size_t)c * h->T * 256, ring + (size_t)c * h->T * 256, (size_t)n_frames * 256 * sizeof(float));
  if (lstm) memcpy(r + L.lstm, lstm, kStateLstmFloats * sizeof(float));
  if (carry) memcpy(r + L.carry, carry, kStateCarryFloats * sizeof(float));
  HIPCHK(h, h->sio.upload(r, (size_t)(ring ? L.total : L.ring), nullptr));   // without a ring: the header and the small sections
  HIPCHK(h, launch_state_import(a, nullptr));
  if (ring && n_frames > 0)
    if (int rc = rebuild_cache(h, nullptr, sid, 1, nullptr)) return rc;
  if (h->rs_hist) {   // the call has no place for the resampler history: the stream's input starts as a new signal
    HIPCHK(h, hipMemsetAsync(h->rs_hist + (size_t)sid * h->rs_rec, 0, (size_t)h->rs_rec * sizeof(float), nullptr));
    HIPCHK(h, hipMemsetAsync(h->rs_started + (size_t)sid * 2, 0, 2 * sizeof(int), nullptr));
  }
  HIPCHK(h, hipStreamSynchronize(nullptr));
  return VAPX_OK;
}

size_t vapx_state_floats(vapx_handle h, int32_t flags) { return h ? state_floats(h, flags) : 0; }

int vapx_export_streams(vapx_handle h, int32_t n, const int32_t* stream_ids, float* dst, int32_t flags, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  { int rc = sio_check(h, "vapx_export_streams", n, stream_ids, dst, flags); if (rc) return rc; }
  hipStream_t st = (hipStream_t)hip_stream;
  const int* ids = nullptr;
  int rc = enter_settled(h, st);
  if (rc || (rc = upload_ids(h, h->sio_ids, n, stream_ids, flags, st, &ids))) return rc;
  const StateLayout L = sio_layout(h, flags);
  if (flags & VAPX_OUT_DEVICE) {   // one gather kernel, no synchronisation
    HIPCHK(h, launch_state_export(sio_args(h, L, dst, ids, n), st));
    return VAPX_OK;
  }
  const size_t rec = (size_t)L.total;
  const bool direct = is_pinned_host(dst);   // vapx_host_alloc memory: the copies land in the caller's block
  int per = 1;
  if ((rc = sio_stage(h, rec, n, !direct, &per))) return rc;
  for (int k0 = 0; k0 < n; k0 += per) {
    const int nb = std::min(per, n - k0);
    StateIoArgs a = sio_args(h, L, h->sio.dev, ids ? ids + k0 : nullptr, nb);
    a.id0 = k0;
    HIPCHK(h, launch_state_export(a, st));
    HIPCHK(h, h->sio.download(dst + (size_t)k0 * rec, (size_t)nb * rec * sizeof(float), st));   // pageable: block by block through the pinned buffer
  }
  HIPCHK(h, hipStreamSynchronize(st));
  return VAPX_OK;
}

int vapx_import_streams(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* src, int32_t flags, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  { int rc = sio_check(h, "vapx_import_streams", n, stream_ids, src, flags); if (rc) return rc; }
  const StateLayout L = sio_layout(h, flags);
  const size_t rec = (size_t)L.total;
  const bool with_cache = (flags & VAPX_STATE_CACHE) != 0, on_host = !(flags & VAPX_OUT_DEVICE);
  if (on_host) {   // every header, before any stream is touched
    const int T = h->T, in_hz = h->in_hz();
    const bool split = (h->cfg.flags & VAPX_FLAG_SPLIT_F16) != 0;
    const StateExpect want{T, h->cfg.frame_hz, in_hz, sio_follower(h), with_cache, split};
    for (int k = 0; k < n; ++k) {
      int32_t hd[SH_WORDS];
      memcpy(hd, src + (size_t)k * rec + L.header, sizeof hd);
      const int bits = hd[SH_BITS];
      switch (state_header_check(hd, want)) {
        case SHF_NONE: break;
        case SHF_MAGIC: return fail(h, VAPX_E_INVAL, "record %d: magic 0x%08x is not a state record (0x%08x)", k, hd[SH_MAGIC], VAPX_STATE_MAGIC);
        case SHF_CTX_FRAMES: return fail(h, VAPX_E_INVAL, "record %d: ctx_frames %d differs from this engine's %d", k, hd[SH_CTX_FRAMES], T);
        case SHF_FRAME_HZ: return fail(h, VAPX_E_INVAL, "record %d: frame_hz %d differs from this engine's %d", k, hd[SH_FRAME_HZ], h->cfg.frame_hz);
        case SHF_ROLE:
          return fail(h, VAPX_E_INVAL, "record %d: content bits 0x%x: %s", k, bits,
                      sio_follower(h) ? "a leader / stand-alone record (LSTM + carry) offered to a trunk follower"
                                      : "a trunk follower's record (no LSTM + carry) offered to a leader / stand-alone engine");
        case SHF_INPUT_RATE:
          return fail(h, VAPX_E_INVAL, "record %d: input_hz %d (content bits 0x%x) differs from this engine's %d: the record %s a resampler history, "
                      "this engine %s", k, hd[SH_INPUT_HZ] ? hd[SH_INPUT_HZ] : 16000, bits, in_hz ? in_hz : 16000,
                      (bits & VAPX_STATE_HAS_RESAMPLE) ? "carries" : "carries no", in_hz ? "keeps one" : "keeps none");
        case SHF_CACHE:
          return fail(h, VAPX_E_INVAL, "record %d: content bits 0x%x: the record %s a Q|K|V cache, the call's flags say it %s", k, bits,
                      (bits & VAPX_STATE_HAS_CACHE) ? "carries" : "carries no", with_cache ? "does" : "does not");
        case SHF_CACHE_PATH:
          return fail(h, VAPX_E_INVAL, "record %d: content bits 0x%x: the Q|K|V cache was made on the %s path, this engine runs the %s path "
                      "(import without VAPX_STATE_CACHE: records without a cache are portable)", k, bits,
                      (bits & VAPX_STATE_CACHE_SPLIT) ? "split-precision" : "fp32", split ? "split-precision" : "fp32");
        case SHF_N_FRAMES: return fail(h, VAPX_E_RANGE, "record %d: n_frames %d outside [0,%d]", k, hd[SH_N_FRAMES], T);
      }
    }
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const int* ids = nullptr;
  int rc = enter_settled(h, st);
  if (rc || (rc = upload_ids(h, h->sio_ids, n, stream_ids, flags, st, &ids))) return rc;
  if (!on_host) {   // one scatter kernel, no synchronisation
    HIPCHK(h, launch_state_import(sio_args(h, L, const_cast<float*>(src), ids, n), st));
  } else {
    const bool direct = is_pinned_host(src);
    int per = 1;
    if ((rc = sio_stage(h, rec, n, !direct, &per))) return rc;
    for (int k0 = 0; k0 < n; k0 += per) {
      const int nb = std::min(per, n - k0);
      HIPCHK(h, h->sio.upload(src + (size_t)k0 * rec, (size_t)nb * rec, st, direct));   // pageable: once the previous block has left the pinned buffer
      StateIoArgs a = sio_args(h, L, h->sio.dev, ids ? ids + k0 : nullptr, nb);
      a.id0 = k0;
      HIPCHK(h, launch_state_import(a, st));
    }
  }
  if (!with_cache && (rc = rebuild_cache(h, ids, 0, n, st))) return rc;
  if (on_host) HIPCHK(h, hipStreamSynchronize(st));
  return VAPX_OK;
}

// Attach to a call in progress: the encoder half of `frames` steps in one call (vapx.h "Prefill").  Per chunk of floor(max_batch / n)
// frames: conv0 over (frame, stream) pairs, the step's conv chain and gx GEMM on that virtual batch, ONE LSTM launch that walks the
// chunk's frames, the layer-0 Q|K|V GEMM of every frame's row and one ring fill.  No transformer layer, no head, no output row.
int vapx_prefill(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* audio, int32_t frames, int32_t flags, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  const char* later = "in this version";
  if (h->trunk || h->orphaned)
    return fail(h, VAPX_E_INVAL, "vapx_prefill is refused on a trunk follower %s: it has no encoder, and its leader's prefill would have to advance "
                "every follower's window and collect state too", later);
  if (!h->followers.empty())
    return fail(h, VAPX_E_INVAL, "vapx_prefill is refused on a trunk leader %s: its followers' windows and collect state would have to advance "
                "over the same frames", later);
  if (h->cls_table)
    return fail(h, VAPX_E_INVAL, "vapx_prefill is refused on an engine with an input-class table %s: every class's resampler history would have to "
                "be advanced over a long block", later);
  if (h->in_hz())
    return fail(h, VAPX_E_INVAL, "vapx_prefill is refused on an engine with an input rate (%d Hz) %s: the resampler history would have to be advanced "
                "over a long block", h->in_hz(), later);
  if (h->n_cls)
    return fail(h, VAPX_E_INVAL, "vapx_prefill is refused on an engine with an input format %s: it takes 16 kHz fp32 samples", later);
  if (n < 1) return fail(h, VAPX_E_RANGE, "vapx_prefill: n=%d outside [1,%d]", n, h->cfg.max_batch);
  if (n > h->cfg.max_batch)
    return fail(h, VAPX_E_INVAL, "vapx_prefill: n=%d exceeds max_batch=%d: a chunk holds at least one frame of every named stream", n, h->cfg.max_batch);
  if (frames < 1) return fail(h, VAPX_E_INVAL, "vapx_prefill: frames=%d, at least one frame is needed", frames);
  if (!audio) return fail(h, VAPX_E_INVAL, "vapx_prefill: null audio");
  if ((uintptr_t)audio & 15) return fail(h, VAPX_E_INVAL, "vapx_prefill: the audio block must be 16-byte aligned");
  if (flags & ~(VAPX_AUDIO_DEVICE | VAPX_IDS_DEVICE)) return fail(h, VAPX_E_INVAL, "vapx_prefill: unknown flag bits 0x%x", flags);
  if (!stream_ids && n > h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "vapx_prefill: n exceeds max_streams");
  hipStream_t st = (hipStream_t)hip_stream;
  const int* ids = nullptr;
  int rc = stream_ids && !(flags & VAPX_IDS_DEVICE) ? check_ids(h, n, stream_ids) : VAPX_OK;
  if (rc || (rc = enter_settled(h, st)) || (rc = upload_ids(h, h->ids, n, stream_ids, flags, st, &ids))) return rc;

  const int hop = h->hop, T = h->T, Fc = prefill_chunk_frames(h->cfg.max_batch, n);
  const bool on_dev = (flags & VAPX_AUDIO_DEVICE) != 0, direct = !on_dev && is_pinned_host(audio);
  const size_t row = (size_t)frames * hop;   // floats of one (stream, channel) row of the caller's block
  const Scratch& sc = h->sc;
  const StateView sv{h->ring, h->ring_qkv, h->h_state, h->c_state, h->carry, h->frames_seen};
  const Weights& w = h->wt;
  for (int f0 = 0; f0 < frames; f0 += Fc) {
    const int fc = std::min(Fc, frames - f0), V = n * fc;
    // the chunk's samples: a device block is read where it lies; host audio travels as [n * 2] rows of [320 | fc * hop] through the
    // step's own staging ([max_batch][2][hop + 320] holds it: n * fc <= max_batch), every row with the 320 samples in front of it -
    // but a call's first chunk, whose prefix is the carry
    const float* src = audio + (size_t)f0 * hop;
    size_t stride = row;
    if (!on_dev) {
      const size_t wrow = VAPX_PAD + (size_t)fc * hop, pre = f0 ? VAPX_PAD : 0, wcopy = pre + (size_t)fc * hop;
      if (direct) {
        HIPCHK(h, hipMemcpy2DAsync(h->audio.dev + (VAPX_PAD - pre), wrow * sizeof(float), src - pre, row * sizeof(float), wcopy * sizeof(float),
                                   (size_t)n * 2, hipMemcpyHostToDevice, st));
      } else {
        HIPCHK(h, hipEventSynchronize(h->audio.evt));   // the previous chunk has left the pinned block
        for (size_t r = 0; r < (size_t)n * 2; ++r)
          memcpy(h->audio.pin + r * wrow + (VAPX_PAD - pre), src - pre + r * row, wcopy * sizeof(float));
        if (!pre)   // the unused prefix slots: defined bytes for the copy
          for (size_t r = 0; r < (size_t)n * 2; ++r) memset(h->audio.pin + r * wrow, 0, VAPX_PAD * sizeof(float));
        HIPCHK(h, hipMemcpyAsync(h->audio.dev, h->audio.pin, (size_t)n * 2 * wrow * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(h, hipEventRecord(h->audio.evt, st));
      }
      src = h->audio.dev + VAPX_PAD;
      stride = wrow;
    }
    Conv0PrefillArgs c0;
    c0.audio = src; c0.row_stride = (long)stride; c0.ids = ids; c0.carry = sv.carry; c0.prefix_in_audio = f0 ? 1 : 0;
    c0.h0 = sc.h0; c0.w = w.conv[0].w; c0.bias = w.conv[0].b; c0.gamma = w.conv[0].g; c0.beta = w.conv[0].beta;
    c0.frames_seen = sv.frames_seen; c0.bhead = f0 ? nullptr : sc.bhead; c0.L = h->L; c0.n = n; c0.T = T;
    { ProfScope ps(h, CLS_CONV0, st); HIPCHK(h, launch_conv0_prefill(c0, V, st)); }
    // what vapx_peek finds afterwards is this chunk: V entries in one group, h2 / h3 only where the chain ran
    h->pass = {V, 1, true, false};
    if ((rc = run_conv_chain(h, sc, V, st))) return rc;
    LstmPrefillArgs la;
    lstm_args(h, sc, sv, la);
    la.ids = ids; la.M = n * 2; la.en = sc.en; la.frames = fc;
    { ProfScope ps(h, CLS_LSTM, st); HIPCHK(h, launch_lstm_prefill(la, st)); }
    if ((long)f0 + fc + T <= frames) continue;   // every frame of this chunk is overwritten by a later one: the LSTM alone had to see it
    {  // layer-0 Q|K|V of every frame's row, as the step makes qkv_new
      GemmArgs g = gemm_args(sc.en, contiguous_rows(256), h->layer[0].wqkv, V * 2, 768, 256, sc.qkv_new, contiguous_rows(768));
      g.W16 = w.l0_wqkv16;
      HIPCHK(h, gemm(h, g, EPI_STORE, st));
    }
    PrefillFillArgs fa;
    fa.ring = sv.ring; fa.ring_qkv = sv.ring_qkv; fa.e = sc.e; fa.qkv_new = sc.qkv_new; fa.ids = ids; fa.bhead = sc.bhead;
    fa.n = n; fa.T = T; fa.fc = fc; fa.f0 = f0; fa.frames = frames;
    fa.frames_seen = sv.frames_seen; fa.carry = sv.carry; fa.tail = src + (size_t)fc * hop - VAPX_PAD; fa.row_stride = (long)stride;
    { ProfScope ps(h, CLS_GATHER, st); HIPCHK(h, launch_prefill_fill(fa, st)); }
  }
  if (!on_dev) HIPCHK(h, hipStreamSynchronize(st));   // the caller's block (and the engine's staging) is free again on return
  return VAPX_OK;
}

int vapx_encode_audio(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* frames, float* e, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  if (h->trunk || h->orphaned) return fail(h, VAPX_E_INVAL, "a trunk follower has no encoder; call the leader");
  if (n < 1 || n > h->cfg.max_batch) return fail(h, VAPX_E_RANGE, "n=%d outside [1,%d]", n, h->cfg.max_batch);
  if (!frames || !e) return fail(h, VAPX_E_INVAL, "null frames/e");
  if (h->cls_table) return fail(h, VAPX_E_INVAL, "vapx_encode_audio takes complete 16 kHz fp32 frames that carry their own carry; this engine has input classes");
  if (h->in_hz()) return fail(h, VAPX_E_INVAL, "vapx_encode_audio takes complete 16 kHz frames that carry their own carry; this engine's input rate is %d Hz", h->in_hz());
  hipStream_t st = (hipStream_t)hip_stream;
  const int* ids = nullptr;
  int rc = stream_ids ? check_ids(h, n, stream_ids) : VAPX_OK;
  if (rc || (rc = enter_settled(h, st)) || (rc = upload_ids(h, h->ids, n, stream_ids, 0, st, &ids))) return rc;
  const StateView sv{h->ring, h->ring_qkv, h->h_state, h->c_state, h->carry, h->frames_seen};
  h->pass.tail_fused = false;
  rc = run_encoder(h, h->sc, sv, n, ids, frames, h->L, false, st);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(e, h->sc.e, (size_t)n * 2 * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
  h->pass.entries = n;
  h->pass.prefill = false;
  return VAPX_OK;
}

int vapx_transformer(vapx_handle h, int32_t n, int32_t rows, const float* x, float* o, float* x12, float* comb,
                     int32_t stage, void* hip_stream) {
  return vapx_transformer_maps(h, n, rows, x, o, x12, comb, stage, nullptr, nullptr, nullptr, hip_stream);
}

int vapx_transformer_maps(vapx_handle h, int32_t n, int32_t rows, const float* x, float* o, float* x12, float* comb,
                          int32_t stage, float* attn, float* self_attn, float* cross_attn, void* hip_stream) {
  if (!h) return VAPX_E_INVAL;
  if (n < 1 || n > h->cfg.max_batch) return fail(h, VAPX_E_RANGE, "n=%d outside [1,%d]", n, h->cfg.max_batch);
  if (rows < 1 || rows > h->T) return fail(h, VAPX_E_RANGE, "rows=%d outside [1,%d]", rows, h->T);
  if (!x) return fail(h, VAPX_E_INVAL, "null x");
  if (stage < 0 || stage > 2) return fail(h, VAPX_E_INVAL, "stage must be 0 (all), 1 (ar_channel) or 2 (ar)");
  if (stage == 1 && (x12 || comb)) return fail(h, VAPX_E_INVAL, "stage 1 produces only o");
  if (stage == 2 && o) return fail(h, VAPX_E_INVAL, "stage 2 does not produce o");
  if (stage == 2 && attn) return fail(h, VAPX_E_INVAL, "stage 2 does not run ar_channel: no attn map");
  if (stage == 1 && (self_attn || cross_attn)) return fail(h, VAPX_E_INVAL, "stage 1 does not run ar: no self_attn / cross_attn maps");
  hipStream_t st = (hipStream_t)hip_stream;
  const int T = h->T;
  const int l_begin = stage == 2 ? 1 : 0, l_end = stage == 1 ? 1 : 4;
  int rc = enter(h);
  if (rc || (rc = join_deferred(h, st))) return rc;   // the stage API shares the step's scratch, and touches no stream state
  hipLaunchKernelGGL(fill_int_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h->sc.bn, rows, n);
  GatherArgs ga;
  memset(&ga, 0, sizeof ga);
  ga.ring = nullptr; ga.e = nullptr; ga.xin = x; ga.ids = nullptr; ga.bn = h->sc.bn; ga.bhead = h->sc.bhead;
  ga.x0 = h->sc.xl[l_begin]; ga.xn = h->sc.xn; ga.gamma = h->layer[l_begin].ln_self_g; ga.beta = h->layer[l_begin].ln_self_b;
  ga.B = n; ga.T = T; ga.rows_in = rows;
  { ProfScope ps(h, CLS_GATHER, st); HIPCHK(h, launch_gather_ln(ga, st)); }
  const MapOut maps{attn, self_attn, cross_attn, rows};
  const bool want_maps = attn || self_attn || cross_attn;
  if ((rc = run_layers(h, h->sc, n, st, l_begin, l_end, false, false, nullptr, want_maps ? &maps : nullptr))) return rc;
  const long nro = (long)n * 2 * rows;
  const unsigned cgrid = (unsigned)((nro * 64 + 255) / 256);
  if (o) hipLaunchKernelGGL(compact_rows_kernel, dim3(cgrid), dim3(256), 0, st, o, h->sc.xl[1], T, rows, nro);
  if (x12) hipLaunchKernelGGL(compact_rows_kernel, dim3(cgrid), dim3(256), 0, st, x12, h->sc.xl[4], T, rows, nro);
  if (comb) {
    rc = run_combinator_all_rows(h, h->sc, n, st);
    if (rc) return rc;
    const long nrc = (long)n * rows;
    // xmid is [n][T][256]; compact with "2 channels" folded: treat as bc = stream
    hipLaunchKernelGGL(compact_rows_kernel, dim3((unsigned)((nrc * 64 + 255) / 256)), dim3(256), 0, st, comb, h->sc.xmid, T, rows, nrc);
  }
  HIPCHK(h, hipGetLastError());
  h->pass.entries = n;
  h->pass.prefill = false;
  return VAPX_OK;
}

int64_t vapx_peek(vapx_handle h, const char* name, float* dst, size_t max_floats) {
  if (!h || !name || !dst) return VAPX_E_INVAL;
  { int rc = quiesce(h); if (rc) return rc; }
  if (!strcmp(name, "guard_violations")) {   // debug: see VAPX_GUARD_ZONES
    dst[0] = guard_enabled() ? (float)guard_violations() : -1.f;
    return 1;
  }
  if (!strcmp(name, "guard_selftest")) {   // debug: the counter above can count.  One byte of an allocation's own trailing canary is changed
    // (inside its hipMalloc: nothing faults), guard_violations() must then say exactly 1; -1 without VAPX_GUARD_ZONES
    dst[0] = -1.f;
    if (!guard_enabled()) return 1;
    unsigned char* probe = nullptr;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, dalloc(&probe, 8));
    hipError_t e = hipMemset(probe + 8, 0x5A, 1);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    const long seen = e == hipSuccess ? guard_violations() : -1;
    dfree(probe);
    HIPCHK(h, e);
    dst[0] = (float)seen;
    return 1;
  }
  const ScratchRow* row = scratch_row_by_peek(name);
  const float* src = row ? (const float*)scratch_ptr(*row, h->sc) : nullptr;   // overlap groups slice every buffer by batch row, so one copy spans them
  if (const char* why = peek_refusal(h->pass, h->cfg.mode, h->ring_direct, h->prune_last, row && !src, name))
    return why == kPeekCombSplit ? fail(h, VAPX_E_INVAL, why, h->pass.groups) : fail(h, VAPX_E_INVAL, why, name, name);
  // "comb": the all-rows combinator of the nod variant, [n][T][256] of xmid
  size_t n = (size_t)h->pass.entries * (!strcmp(name, "comb") ? (size_t)h->T * 256 : row->per_slot(*h));
  if (n > max_floats) n = max_floats;
  HIPCHK(h, hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToHost));
  return (int64_t)n;
}

int vapx_profile_enable(vapx_handle h, uint32_t class_mask) {
  if (!h) return VAPX_E_INVAL;
  h->prof_mask = class_mask;
  return VAPX_OK;
}

int vapx_profile_read(vapx_handle h, double* total_ms, int64_t* launches, int32_t n_classes) {
  if (!h || !total_ms || !launches) return VAPX_E_INVAL;
  if (int rc = enter(h)) return rc;
  HIPCHK(h, hipDeviceSynchronize());
  for (int i = 0; i < n_classes; ++i) { total_ms[i] = 0.0; launches[i] = 0; }
  for (auto& r : h->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess && r.cls < n_classes) { total_ms[r.cls] += ms; launches[r.cls] += 1; }
    h->prof_pool.push_back(r.a);
    h->prof_pool.push_back(r.b);
  }
  h->prof_recs.clear();
  return VAPX_OK;
}

int vapx_vap_head(vapx_handle h, int64_t rows, const float* x, float* logits, void* hip_stream) {
  if (!h || !x || !logits || rows < 1) return VAPX_E_INVAL;
  if (h->cfg.mode != VAPX_MODE_VAP) return fail(h, VAPX_E_INVAL, "this weight set has no vap_head (bc / nod variant)");
  if (int rc = enter(h)) return rc;
  GemmArgs g = gemm_args(x, contiguous_rows(256), h->wt.head_w, (int)rows, 256, 256, logits, contiguous_rows(256));
  g.bias = h->wt.head_b;
  HIPCHK(h, launch_gemm_f32(g, EPI_STORE, 0, (hipStream_t)hip_stream));
  return VAPX_OK;
}

int vapx_va_classifier(vapx_handle h, int64_t rows, const float* x, float* y, void* hip_stream) {
  if (!h || !x || !y || rows < 1) return VAPX_E_INVAL;
  if (int rc = enter(h)) return rc;
  hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, x, h->wt.vad_w, h->wt.vad_b, y, (long)rows);
  HIPCHK(h, hipGetLastError());
  return VAPX_OK;
}

int vapx_aux_head(vapx_handle h, int32_t which, int64_t rows, const float* x, float* y, void* hip_stream) {
  if (!h || !x || !y || rows < 1) return VAPX_E_INVAL;
  // aux.w rows: bc variant = bc_head rows 0..2; nod variant = nod_head rows 0..3, bc_head row 4 (weights.pack_blob)
  int row0, nout;
  if (h->cfg.mode == VAPX_MODE_BC && which == VAPX_AUX_BC_HEAD) { row0 = 0; nout = 3; }
  else if (h->cfg.mode == VAPX_MODE_NOD && which == VAPX_AUX_BC_HEAD) { row0 = 4; nout = 1; }
  else if (h->cfg.mode == VAPX_MODE_NOD && which == VAPX_AUX_NOD_HEAD) { row0 = 0; nout = 4; }
  else return fail(h, VAPX_E_INVAL, "this weight set has no such head (bc_head: bc / nod variants, nod_head: nod variant)");
  if (int rc = enter(h)) return rc;
  hipLaunchKernelGGL(rowheads_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, x, h->wt.aux_w + row0 * 256,
                     h->wt.aux_b + row0, y, (long)rows, nout);
  HIPCHK(h, hipGetLastError());
  return VAPX_OK;
}

// one class as the input kernel reads it; false: a rate or format that does not exist, named in the engine's error text
static bool input_class_geom(vapx_engine* h, int hz, int fmt, const char* who, InputClassGeom* out) {
  ResampleGeom g = {};   // 16 kHz: orig = 0, no window
  if (hz != 16000 && !resample_geometry(hz, &g)) {
    fail(h, VAPX_E_INVAL, "%sinput rate %d Hz: supported are 8000, 16000, 32000 and 48000", who, hz);
    return false;
  }
  if (fmt < VAPX_PCM_F32 || fmt > VAPX_PCM_ALAW) {
    fail(h, VAPX_E_INVAL, "%sinput format %d: known are 0 (f32), 1 (s16), 2 (mulaw) and 3 (alaw)", who, fmt);
    return false;
  }
  *out = {g.orig, g.nnew, g.width, g.K, g.d, g.H, hz / h->cfg.frame_hz, fmt};
  return true;
}

// (Re)build the engine's input state for the classes tab[0 .. n): the history and the `started` flags for the largest H, the 16 kHz output,
// staging for host audio where the largest slot exceeds what `audio` holds, and the slot descriptors of a caller's table.  A buffer whose
// size does not change is kept with its contents: a format set after a rate keeps the history.  On an allocation failure the engine stays
// as it was and nothing leaks.  `what` names the state in the error text.
static int build_input(vapx_engine* h, const InputClassGeom* tab, int n, bool table, const char* what) {
  if (int rc = enter(h)) return rc;
  HIPCHK(h, hipDeviceSynchronize());
  const size_t S = h->cfg.max_streams, B = h->cfg.max_batch;
  int Hmax = 0;
  size_t slot_max = 0;
  for (int i = 0; i < n; ++i) {
    Hmax = std::max(Hmax, tab[i].H);
    slot_max = std::max(slot_max, (size_t)2 * tab[i].hop_in * (size_t)pcm_bytes_per_sample(tab[i].fmt));
  }
  const int rec = (2 * Hmax + 3) & ~3;
  const int row = !table && tab[0].orig == 0 ? h->L : h->hop;   // a uniform 16 kHz engine may be stepped with full frames (never a larger block than `audio` holds)
  const size_t stage_floats = B * slot_max / sizeof(float);     // staging for host audio: the largest slot in every batch slot
  float *hist = nullptr, *rout = nullptr;
  int* started = nullptr;
  Staged<int> slots;
  hipError_t e = hipSuccess;
  if (rec != h->rs_rec) {
    e = dalloc(&hist, S * (size_t)rec);
    if (e == hipSuccess) e = dalloc(&started, S * 2);
  }
  if (e == hipSuccess && row != h->rs_row) e = dalloc(&rout, B * 2 * (size_t)row);
  if (e == hipSuccess && table) e = slots.reserve(B * 2, true);
  if (e == hipSuccess) e = h->audio.reserve(stage_floats, true);   // the last that can fail: a larger block alone changes nothing
  if (e != hipSuccess) {   // the engine stays as it was
    (void)hipGetLastError();
    dfree(hist); dfree(started); dfree(rout);
    slots.release();
    return fail(h, e == hipErrorOutOfMemory ? VAPX_E_NOMEM : VAPX_E_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  if (hist) { dfree(h->rs_hist); dfree(h->rs_started); h->rs_hist = hist; h->rs_started = started; h->rs_rec = rec; }
  if (rout) { dfree(h->rs_out); h->rs_out = rout; h->rs_row = row; }
  if (table) {
    h->cls_slots = slots;
    h->cls_slots_host.assign(B, InputSlot{0, 0});
    h->stream_cls.assign(S * 2, 0);
  }
  memcpy(h->cls, tab, (size_t)n * sizeof *tab);
  h->cls_lds = input_classes_lds_floats(tab, n);
  h->n_cls = n;
  h->cls_table = table;
  return VAPX_OK;
}

int vapx_set_input_rate(vapx_handle h, int32_t input_hz) {
  if (!h) return VAPX_E_INVAL;
  InputClassGeom g;
  if (!input_class_geom(h, input_hz, h->in_fmt(), "", &g)) return VAPX_E_INVAL;   // the class of a uniform engine: this rate, the format it has
  if (h->trunk || h->orphaned) return fail(h, VAPX_E_INVAL, "a trunk follower takes no audio: set the input rate on the leader");
  if (h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has input classes (vapx_set_input_classes): the rate is each class's own");
  if (h->tick != 0 || h->in_hz()) return fail(h, VAPX_E_INVAL, "set the input rate once, on a freshly created engine, before its first step");
  if (input_hz == 16000) return VAPX_OK;
  char what[64];
  snprintf(what, sizeof what, "resampler state for %d Hz", input_hz);
  return build_input(h, &g, 1, false, what);
}

int32_t vapx_get_input_rate(vapx_handle h) { return !h ? VAPX_E_INVAL : (h->in_hz() ? h->in_hz() : 16000); }

int vapx_set_input_format(vapx_handle h, int32_t format) {
  if (!h) return VAPX_E_INVAL;
  InputClassGeom g;
  if (!input_class_geom(h, h->in_hz() ? h->in_hz() : 16000, format, "", &g)) return VAPX_E_INVAL;   // this format, the rate it has
  if (h->trunk || h->orphaned) return fail(h, VAPX_E_INVAL, "a trunk follower takes no audio: set the input format on the leader");
  if (h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has input classes (vapx_set_input_classes): the format is each class's own");
  if (h->tick != 0 || h->in_fmt()) return fail(h, VAPX_E_INVAL, "set the input format once, on a freshly created engine, before its first step");
  if (format == VAPX_PCM_F32) return VAPX_OK;
  char what[64];
  snprintf(what, sizeof what, "decoded-input buffer for input format %d", format);
  return build_input(h, &g, 1, false, what);
}

int32_t vapx_get_input_format(vapx_handle h) { return !h ? VAPX_E_INVAL : h->in_fmt(); }

int vapx_set_input_classes(vapx_handle h, int32_t n, const vapx_input_class* classes) {
  if (!h) return VAPX_E_INVAL;
  if (h->trunk || h->orphaned) return fail(h, VAPX_E_INVAL, "a trunk follower takes no audio: set the input classes on the leader");
  if (h->n_cls && !h->cls_table)
    return fail(h, VAPX_E_INVAL, "this engine has an input %s of its own (vapx_set_input_%s): input classes replace both calls, they do not combine",
                h->in_hz() ? "rate" : "format", h->in_hz() ? "rate" : "format");
  if (h->tick != 0 || h->cls_table) return fail(h, VAPX_E_INVAL, "set the input classes once, on a freshly created engine, before its first step");
  if (n < 1 || n > VAPX_MAX_INPUT_CLASSES || !classes)
    return fail(h, VAPX_E_INVAL, "n = %d input classes: the table holds 1 .. %d", n, VAPX_MAX_INPUT_CLASSES);
  InputClassGeom tab[VAPX_MAX_INPUT_CLASSES] = {};
  size_t slot_max = 0;
  for (int i = 0; i < n; ++i) {
    const int hz = classes[i].input_hz, fmt = classes[i].format;
    char who[16];
    snprintf(who, sizeof who, "class %d: ", i);
    if (!input_class_geom(h, hz, fmt, who, &tab[i])) return VAPX_E_INVAL;
    for (int j = 0; j < i; ++j)
      if (classes[j].input_hz == hz && classes[j].format == fmt)
        return fail(h, VAPX_E_INVAL, "classes %d and %d are equal (format %d at %d Hz): a duplicate entry", j, i, fmt, hz);
    slot_max = std::max(slot_max, (size_t)2 * tab[i].hop_in * (size_t)pcm_bytes_per_sample(fmt));
  }
  if ((size_t)h->cfg.max_batch * slot_max > 0xFFFFFFFFull)
    return fail(h, VAPX_E_INVAL, "max_batch %d x the largest slot (%zu bytes) passes 4 GiB: a slot's offset in the packed block is 32 bits", h->cfg.max_batch, slot_max);
  char what[64];
  snprintf(what, sizeof what, "state and staging for %d input classes", n);
  const int rc = build_input(h, tab, n, true, what);
  if (rc == VAPX_OK) memcpy(h->cls_pub, classes, (size_t)n * sizeof *classes);
  return rc;
}

int32_t vapx_get_input_classes(vapx_handle h, vapx_input_class* out, int32_t max) {
  if (!h) return VAPX_E_INVAL;
  for (int i = 0; out && i < h->tab_cls() && i < max; ++i) out[i] = h->cls_pub[i];
  return h->tab_cls();
}

int vapx_set_stream_class(vapx_handle h, int32_t sid, int32_t cls) {
  if (!h) return VAPX_E_INVAL;
  if (!h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has no input classes (vapx_set_input_classes)");
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id %d out of range [0,%d)", sid, h->cfg.max_streams);
  if (cls < 0 || cls >= h->tab_cls()) return fail(h, VAPX_E_RANGE, "input class %d out of range [0,%d)", cls, h->tab_cls());
  // a new class is a new signal: the carry-only request of vapx_reset_carry (carry, resampler history, started flags), applied by the next
  // step before it touches any state; that step is also the first to build a slot descriptor from the stream's class, which lives on the host
  const int rc = vapx_reset_carry(h, sid);
  if (rc == VAPX_OK) h->stream_cls[(size_t)2 * sid] = h->stream_cls[(size_t)2 * sid + 1] = cls;
  return rc;
}

int32_t vapx_get_stream_class(vapx_handle h, int32_t sid) {
  if (!h) return VAPX_E_INVAL;
  if (!h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has no input classes (vapx_set_input_classes)");
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id %d out of range [0,%d)", sid, h->cfg.max_streams);
  const int32_t* c = &h->stream_cls[(size_t)2 * sid];
  if (c[0] != c[1])
    return fail(h, VAPX_E_INVAL, "stream %d has channel classes (%d, %d), not one class: ask vapx_get_stream_channel_classes", sid, c[0], c[1]);
  return c[0];
}

int vapx_set_stream_channel_classes(vapx_handle h, int32_t sid, int32_t c1, int32_t c2) {
  if (!h) return VAPX_E_INVAL;
  if (!h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has no input classes (vapx_set_input_classes)");
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id %d out of range [0,%d)", sid, h->cfg.max_streams);
  for (int c = 0; c < 2; ++c) {
    const int cls = c ? c2 : c1;
    if (cls < 0 || cls >= h->tab_cls()) return fail(h, VAPX_E_RANGE, "input class %d of channel %d out of range [0,%d)", cls, c + 1, h->tab_cls());
  }
  // the request of vapx_set_stream_class: the carry, the history and the started flags of BOTH channels restart, also where only one leg's
  // class changes (the 320-sample carry and the reset list are per stream)
  const int rc = vapx_reset_carry(h, sid);
  if (rc == VAPX_OK) { h->stream_cls[(size_t)2 * sid] = c1; h->stream_cls[(size_t)2 * sid + 1] = c2; }
  return rc;
}

int vapx_get_stream_channel_classes(vapx_handle h, int32_t sid, int32_t out[2]) {
  if (!h) return VAPX_E_INVAL;
  if (!out) return fail(h, VAPX_E_INVAL, "null out");
  if (!h->cls_table) return fail(h, VAPX_E_INVAL, "this engine has no input classes (vapx_set_input_classes)");
  if (sid < 0 || sid >= h->cfg.max_streams) return fail(h, VAPX_E_RANGE, "stream id %d out of range [0,%d)", sid, h->cfg.max_streams);
  out[0] = h->stream_cls[(size_t)2 * sid];
  out[1] = h->stream_cls[(size_t)2 * sid + 1];
  return VAPX_OK;
}

int64_t vapx_input_row_bytes(vapx_handle h, int32_t cls) {
  if (!h || cls < 0 || cls >= h->tab_cls()) return 0;
  return (int64_t)h->cls_row_bytes(cls);
}

int64_t vapx_input_slot_bytes(vapx_handle h, int32_t cls) {
  if (!h || cls < 0 || cls >= h->tab_cls()) return 0;
  return (int64_t)h->cls_slot_bytes(cls);
}

int vapx_pcm_decode(int32_t format, int64_t n, const void* src, float* dst, void* hip_stream) {
  if (!src || !dst || n < 1 || n > ((int64_t)1 << 40) || format < VAPX_PCM_S16 || format > VAPX_PCM_ALAW) return VAPX_E_INVAL;
  // dword loads; the stores are 16 bytes for G.711 and 8 for s16, which would do with an 8-byte aligned dst: one documented rule (vapx.h) for
  // all three formats instead, which every device allocation meets
  if (((uintptr_t)src & 3) || ((uintptr_t)dst & 15)) return VAPX_E_INVAL;
  (void)hipGetLastError();
  return launch_pcm_decode(format, (long)n, src, dst, (hipStream_t)hip_stream) == hipSuccess ? VAPX_OK : VAPX_E_HIP;
}

int vapx_resample(int32_t input_hz, int64_t rows, int64_t n_in, const float* x, float* y, void* hip_stream) {
  if (!x || !y || rows < 1 || n_in < 1 || n_in > ((int64_t)1 << 40)) return VAPX_E_INVAL;
  (void)hipGetLastError();
  if (input_hz == 16000)
    return hipMemcpyAsync(y, x, (size_t)rows * (size_t)n_in * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream) == hipSuccess ? VAPX_OK : VAPX_E_HIP;
  ResampleGeom g = {};
  if (!resample_geometry(input_hz, &g)) return VAPX_E_INVAL;
  return launch_resample_whole(g, (long)rows, (long)n_in, x, y, (hipStream_t)hip_stream) == hipSuccess ? VAPX_OK : VAPX_E_HIP;
}

int vapx_softmax256(int64_t rows, const float* x, float* y, void* hip_stream) {
  if (!x || !y || rows < 1) return VAPX_E_INVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(softmax256_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, x, y, (long)rows);
  return hipGetLastError() == hipSuccess ? VAPX_OK : VAPX_E_HIP;
}

int vapx_aggregate(int64_t rows, const float* probs, int32_t from_bin, int32_t to_bin, float* out, void* hip_stream) {
  if (!probs || !out || rows < 1 || from_bin < 0 || to_bin > 3 || from_bin > to_bin) return VAPX_E_INVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, probs, out, (long)rows, from_bin, to_bin);
  return hipGetLastError() == hipSuccess ? VAPX_OK : VAPX_E_HIP;
}

int vapx_gemm(void* hip_stream, int32_t M, int32_t N, int32_t K, const float* A, const float* W, float* C, int32_t epi,
              const float* bias, const float* gamma, const float* beta, const float* resid, float* C2, int32_t tile_rows) {
  (void)hipGetLastError();
  GemmArgs g = gemm_args(A, contiguous_rows(K), W, M, N, K, C, contiguous_rows(N));
  g.bias = bias; g.gamma = gamma; g.beta = beta; g.resid = resid; g.C2 = C2;
  hipError_t e = launch_gemm_f32(g, epi, tile_rows, (hipStream_t)hip_stream);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? VAPX_E_INVAL : VAPX_E_HIP, "vapx_gemm: %s", hipGetErrorString(e));
  return VAPX_OK;
}

int vapx_gemm_tile_rows(int32_t M, int32_t N, int32_t K, int32_t epi) { return gemm_tile_rows(M, N, K, epi); }

}  // extern "C"
