// Native many-stream TCP front-end of libvapx (include/vapx.h, "vapx_ingest_*"), host code only.
//
// Reference being replaced: proc_serv_in / proc_serv_out / proc_serv_out_dist, rvap/vap_main/vap_main.py:338-457, and the
// per-sample Python codec rvap/common/util.py:52-237 — one dialogue per process there, thousands per process here.
//
//   rx threads (epoll)      recv -> decode f64 pairs -> per-stream frame buffers (f32 staging in page-locked memory + the
//                           f64 echo the result packet carries); a complete frame is queued for the tick thread
//   tick thread             batches the ready frames (ragged), vapx_step (host in / host out), hands rows to the senders
//   tx threads              encode header / tail, sendmsg() with the echo arrays as iovecs (no copy), free the frame buffer
//
// Input classes (vapx_ingest_config.input_classes; vapx.h "Input classes"): one input port per class; a connection accepted on class c's port
// makes its slot a stream of class c, whose geometry (InGeo: format, hop, packet size) every thread takes from the slot or from the queued
// frame instead of from the front-end; the tick packs the ready frames' slots back to back, which is the packed block the engine takes.
// A front-end without a table is the one-class case: one geometry, geo[0], one input port, and every slot is of it; only the public calls
// tell it from a table of one (vapx_ingest::cls_table).
// Pair ports (vapx_ingest_config.pair_ports; vapx.h CHANNEL CLASSES): a connection on pair port (c1, c2) is a dialogue whose channel 1 is of
// class c1 and whose channel 2 of c2.  Its packets are planar (channel 1's 10 ms, then channel 2's), its frame buffer holds
// channel 1's row and then channel 2's, each in its own class's staging form, which is the engine's slot.  A slot of any other port is
// the case c1 == c2 of that layout.
//
// A raw input format (vapx_ingest_config.input_format: s16, mulaw, alaw; vapx.h "Input format"): the receive threads only de-interleave
// the samples into the staging as they are (no cast, no f32 staging, no f64 echo copy), the tick hands the raw block to the step, whose
// engine decodes on the device, and a sender expands the frame's echo from the raw staging by pcm_tables.h when it encodes the packet.
//
// Every stream owns NBUF frame buffers (filling / waiting / in flight / being sent + slack), so reception never waits for the GPU
// unless a sender outruns the engine by four whole frames; then the connection is paused (TCP back-pressure), never dropped.
#include <arpa/inet.h>
#include <errno.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <pthread.h>
#include <sched.h>
#include <sys/epoll.h>
#include <sys/eventfd.h>
#include <sys/resource.h>
#include <sys/socket.h>
#include <sys/uio.h>
#include <sys/un.h>
#include <poll.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vapx.h"
#include "pcm_tables.h"

// the engine's group entry points: weak here, so the front-end still links into a program that stubs only the single-model
// engine calls (tests/native); vapx_ingest_open_group says so if they are missing
#pragma weak vapx_step_group
#pragma weak vapx_group_wire_floats
// the engine's input rate (vapx_set_input_rate): weak for the same reason; a program without it serves 16 kHz
#pragma weak vapx_get_input_rate
// the engine's input format (vapx_set_input_format): weak for the same reason; a program without it takes fp32
#pragma weak vapx_get_input_format
// the engine's input classes (vapx_set_input_classes): weak for the same reason; a program without them has no table
#pragma weak vapx_get_input_classes
#pragma weak vapx_set_stream_class
#pragma weak vapx_set_stream_channel_classes

namespace {

constexpr int NBUF = 5;   // frame buffers per stream: filling + waiting + in flight + two of slack for a client that bursts after a stall
constexpr int MAX_MODELS = 3;                 // output ports of one front-end: a trunk group serves up to vap + bc + nod
constexpr int PAIR_BYTES = 16;                 // one sample of both channels: f64 ch1, f64 ch2 (util.py:52-62)
// raw input formats (vapx.h "Input format"): the 16-bit linear value of a sample; its value is that times 2^-15, exact in f32 and f64
constexpr int16_t kMulaw[256] = {VAPX_PCM_MULAW_TABLE};
constexpr int16_t kAlaw[256] = {VAPX_PCM_ALAW_TABLE};
enum BufState : int { B_FREE = 0, B_FILLING = 1, B_READY = 2, B_INFLIGHT = 3 };

// Timed condition wait.  Under ThreadSanitizer the wait goes through system_clock (pthread_cond_timedwait): gcc-11's libtsan does
// not intercept pthread_cond_clockwait, loses the unlock inside it and then reports every access under that mutex as a race.
template <class Rep, class Period>
inline void cv_wait_for(std::condition_variable& cv, std::unique_lock<std::mutex>& lk, std::chrono::duration<Rep, Period> d) {
#if defined(__SANITIZE_THREAD__)
  cv.wait_until(lk, std::chrono::system_clock::now() + d);
#else
  cv.wait_for(lk, d);
#endif
}

double mono_now() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
double unix_now() {
  timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

inline void atomic_max(std::atomic<int64_t>& a, int64_t v) {
  int64_t m = a.load(std::memory_order_relaxed);
  while (v > m && !a.compare_exchange_weak(m, v, std::memory_order_relaxed)) {}
}

// ---- codec ---------------------------------------------------------------------------------------
inline void put_u32(uint8_t*& p, uint32_t v) { memcpy(p, &v, 4); p += 4; }   // little-endian host (x86-64 / the GPU box)
inline void put_f64(uint8_t*& p, double v) { memcpy(p, &v, 8); p += 8; }

// number of head values after the echo blocks, by mode
int tail_bytes(int mode, int n_rows_pbc) {
  if (mode == VAPX_MODE_VAP) return 3 * (4 + 16);
  if (mode == VAPX_MODE_BC) return 2 * (4 + 8);
  return (4 + 8 * n_rows_pbc) + 3 * (4 + 8);
}

// heads of one out row -> tail of the packet (after "u32 n | x2"); returns bytes written
int encode_tail(int mode, const float* row, uint8_t* dst, int max_rows = 256) {
  uint8_t* p = dst;
  if (mode == VAPX_MODE_VAP) {            // u32 2 | p_now | u32 2 | p_future | u32 2 | vad   (util.py:134-141)
    for (int blk = 0; blk < 3; ++blk) {
      put_u32(p, 2);
      put_f64(p, (double)row[blk * 2]);
      put_f64(p, (double)row[blk * 2 + 1]);
    }
  } else if (mode == VAPX_MODE_BC) {      // u32 1 | p_bc_react | u32 1 | p_bc_emo            (util.py:193-211)
    put_u32(p, 1); put_f64(p, (double)row[VAPX_OUT_AUX + 1]);
    put_u32(p, 1); put_f64(p, (double)row[VAPX_OUT_AUX + 2]);
  } else {                                // u32 n | p_bc rows | 3 x (u32 1 | p)              (util.py:213-237, vap_nod_main.py:276)
    // clamped to the tail buffer's 256 rows: a step function of vapx_ingest_open_fn that leaves the column unset must not
    // turn into an out-of-bounds write here (vapx_wire_encode_result validates the same range)
    int n = (int)row[VAPX_OUT_NVALID];
    n = n < 0 ? 0 : (n > max_rows ? max_rows : n);   // (max_rows: a wire row holds ctx_frames of them, an output row 256)
    put_u32(p, (uint32_t)n);
    for (int i = 0; i < n; ++i) put_f64(p, (double)row[VAPX_OUT_LOGITS + i]);
    for (int k = 1; k <= 3; ++k) { put_u32(p, 1); put_f64(p, (double)row[VAPX_OUT_AUX + k]); }
  }
  return (int)(p - dst);
}

struct Hist {   // log2-spaced latency histogram, 8 sub-buckets per octave from 1 us
  static constexpr int N = 8 * 27;
  std::atomic<int64_t> b[N];
  std::atomic<int64_t> cnt{0};
  std::atomic<int64_t> sum_us{0};
  std::atomic<int64_t> max_us{0};
  Hist() { for (auto& x : b) x = 0; }
  void add(double sec) {
    double us = sec * 1e6;
    if (us < 1.0) us = 1.0;
    int k = (int)(log2(us) * 8.0);
    if (k >= N) k = N - 1;
    b[k].fetch_add(1, std::memory_order_relaxed);
    cnt.fetch_add(1, std::memory_order_relaxed);
    sum_us.fetch_add((int64_t)us, std::memory_order_relaxed);
    int64_t m = max_us.load(std::memory_order_relaxed), v = (int64_t)us;
    while (v > m && !max_us.compare_exchange_weak(m, v, std::memory_order_relaxed)) {}
  }
  double pct(double q) const {
    int64_t total = cnt.load(), acc = 0;
    if (total == 0) return 0.0;
    int64_t want = (int64_t)ceil(q * (double)total);
    for (int k = 0; k < N; ++k) {
      acc += b[k].load();
      if (acc >= want) return exp2((k + 1) / 8.0) * 1e-3;   // upper edge of the bucket, ms
    }
    return (double)max_us.load() * 1e-3;
  }
  void clear() { for (auto& x : b) x = 0; cnt = 0; sum_us = 0; max_us = 0; }
};

// the geometry of an input class (a front-end without a table has one).  The sample sizes are derived here and nowhere else
struct InGeo {
  // wire format: VAPX_PCM_F32 = the reference's f64 pairs, cast to f32 on the host (the engine's format is f32); S16 / MULAW / ALAW = raw
  // samples, staged as they are and handed to the step as they are (the engine decodes: vapx_set_input_format)
  int fmt = VAPX_PCM_F32;
  int in_hz = 16000;
  int hop = 0;                             // samples per channel and frame on the wire = in_hz / frame_hz (the engine resamples: vapx_set_input_rate)
  int bps() const { return fmt == VAPX_PCM_F32 ? 4 : fmt == VAPX_PCM_S16 ? 2 : 1; }   // bytes per sample of the staging
  int wire_bps() const { return fmt ? bps() : 8; }                 // bytes per sample on the wire: f64 for an F32 class
  size_t row_bytes() const { return (size_t)hop * bps(); }         // one channel's row of the staging
  size_t frame_bytes() const { return 2 * row_bytes(); }           // a frame of the staging = a slot of the step's block
  size_t wire_row() const { return (size_t)hop * wire_bps(); }     // one channel's samples of a frame on the wire
};

// an input port: its listen socket (-1: a passive shard listens on nothing), the port bound, and what a connection accepted on it is
struct InPort {
  int lsock = -1, port = 0;
  int cls = 0, cls2 = 0;                   // the classes of channel 1 and channel 2: equal but on a pair port
  bool planar = false;                     // a pair port: planar 10 ms packets
};

struct Slot {
  int fd_in = -1;
  int cls = 0;                             // index into vapx_ingest::geo; written at adoption, before the socket joins an epoll set
  int cls2 = 0;                            // channel 2's class: cls unless the connection came in on a pair port
  bool planar = false;                     // a pair port's connection: planar 10 ms packets
  std::atomic<uint32_t> gen{0};           // bumped per connection: queued frames of a dead connection are dropped (read by the tick thread)
  std::atomic<int> state[NBUF];
  double t_ready[NBUF] = {};
  int wbuf = -1, fill = 0;                // rx thread only: the frame buffer being filled and the wire bytes of its frame taken so far
  uint8_t partial[PAIR_BYTES];            // the head of an f64 sample (pair) split across two reads; its bytes are counted in `fill`
  std::vector<uint8_t> backlog;           // bytes received while no buffer was free
  int lowat = 0;                          // rx thread only: SO_RCVLOWAT currently set on fd_in (0 = the kernel default)
  std::atomic<bool> paused{false};        // written by the slot's rx / accept thread, read by whoever frees a buffer
  std::mutex lmu;                         // guards listeners
  std::vector<int> listeners[MAX_MODELS]; // per output port (model); a single-model front-end uses [0] only
  // VAPX_INGEST_DEBUG bookkeeping (relaxed counters, printed at close): where do a stream's frames go?
  std::atomic<int64_t> dbg_ready{0}, dbg_sent{0}, dbg_nolistener{0};
  double dbg_t_first_ready = 0, dbg_t_attach = 0, dbg_t_first_sent = 0;
  Slot() { for (auto& s : state) s = B_FREE; }
};

struct Ready { int slot; int buf; uint32_t gen; double t; int cls, cls2; };   // the slot's channel classes when the frame was completed
struct ResetReq { int slot; int carry_only; int cls, cls2; };          // cls >= 0: the connection's input classes (a front-end with a table)

struct Job {                               // one tick's rows on their way out
  int n = 0;
  std::vector<Ready> rows;
  float* out = nullptr;                    // pinned; [max_batch][VAPX_OUT_STRIDE], or a trunk group's wire block [model][n][wire floats]
  std::vector<uint8_t> bad;                // per row: some model's status is 1, not finite (no packet on any port)
  double t_unix = 0;
  std::vector<std::vector<int>> part;      // row indices per sender thread: slot % X — a stream is always sent by the same thread
  int senders_done = 0;                    // sender threads that are through with this job (under job_mu)
  bool busy = false;
};

// one output port: a model's listen socket, its framing and its listener placement (fewest listeners, lowest slot first)
struct OutPort {
  int mode = 0;
  int wf = VAPX_OUT_STRIDE;                // floats per row of this model in a job's block
  size_t off = 0;                          // floats per stream in front of this model's rows (the block is model-major)
  int R = 1;                               // leader hops per frame of this model (a trunk follower slower than its leader: > 1)
  // R > 1: the f64 echo of the leader hops of each dialogue's frame in the making.  Touched only by the slot's sender thread
  // (slot % X), which sees a slot's rows in tick order.
  std::vector<double> hist;                // [S][R-1][2][hop]
  std::vector<int> hist_n;                 // [S] hops held
  std::vector<uint32_t> hist_gen;          // [S] the connection they belong to: a new connection starts with an empty history
  int lsock = -1, port = 0;
  std::vector<int> out_all;                // broadcast listeners (under slots_mu)
  std::vector<int> lcount;                 // listeners per slot (under slots_mu)
  int lmin = 0, lcursor = 0;               // fewest listeners on any slot; lowest slot that may still have that few
};

}  // namespace

struct vapx_ingest {
  vapx_ingest_config cfg;
  vapx_ingest_step_fn step = nullptr;
  vapx_ingest_reset_fn reset = nullptr;
  void* user = nullptr;
  vapx_handle engine = nullptr;
  int S = 0, max_batch = 0, hz = 0;
  // The input: geo[c] is class c's geometry, n_cls >= 1 of them.  cls_table: the caller (or the engine) gave a table; without one the
  // engine's rate and format are the one class, and the public calls report no classes (tab_cls).  in_ports: one per class, then the pair
  // ports; without a table the one input port.  frame_stride / echo_stride: bytes / doubles between two frame buffers, sized for the largest class
  bool cls_table = false;
  int n_cls = 1;
  int tab_cls() const { return cls_table ? n_cls : 0; }
  InGeo geo[VAPX_MAX_INPUT_CLASSES];
  vapx_input_class cls_pub[VAPX_MAX_INPUT_CLASSES] = {};
  int n_in = 0;
  InPort in_ports[VAPX_MAX_INPUT_CLASSES + VAPX_MAX_PAIR_PORTS];
  size_t frame_stride = 0, echo_stride = 0;
  std::vector<int32_t> tick_cls;           // [S][2] tick thread only: a stream's channel classes as the engine (or the step function) knows them
  void (*set_class)(void* user, int32_t stream_id, int32_t cls, int32_t cls2) = nullptr;   // tick thread: vapx_set_stream_class / _channel_classes on the engine
  size_t frame_bytes(int c1, int c2) const { return geo[c1].row_bytes() + geo[c2].row_bytes(); }   // a slot of the step's block
  // where channel 2's f64 echo starts in a frame's echo buffer: behind channel 1's [hop] for one class; half the buffer (the largest f64
  // hop) where the classes differ, whatever channel 1's class is
  size_t echo_ch2(int c1, int c2) const { return c1 == c2 ? (size_t)geo[c1].hop : echo_stride / 2; }
  int M = 1;                               // models = output ports (> 1: a trunk group, `step` fills wire blocks)
  OutPort ports[MAX_MODELS];
  size_t row_floats = VAPX_OUT_STRIDE;     // floats per stream in a job's block, all models
  int cfg_ports_out[MAX_MODELS] = {0, 0, 0};   // requested ports of the followers ([0] unused: cfg.port_out)
  bool broadcast = false;
  int R = 2, X = 2;

  std::unique_ptr<Slot[]> slots;
  float* stage = nullptr;                  // pinned [S][NBUF][2][hop] f32, or raw samples of bps bytes
  std::vector<double> echo;                // [S][NBUF][2][hop] f64; a raw format keeps none: the echo is expanded from `stage` when a packet is encoded
  float* batch_audio = nullptr;            // pinned [max_batch][2][hop], f32 or raw
  std::vector<int32_t> batch_ids;
  Job jobs[2];

  std::vector<int> ep;                     // epoll fd per rx thread
  std::vector<int> wake;                   // eventfd per rx thread (resume / stop)
  std::vector<std::thread> rx_threads, tx_threads;
  std::thread tick_thread;
  std::atomic<bool> stop{false};

  std::mutex slots_mu;                     // slot allocation, the ports' out_all and listener bookkeeping
  int free_hint = 0;                       // no input slot below this one is free (under slots_mu): adoption is O(1) amortised, not a scan of S slots
  int ep_accept = -1;                      // the accept thread's epoll (listen sockets only)
  std::thread accept_thread;
  std::mutex ready_mu;
  std::condition_variable ready_cv;
  std::vector<Ready> ready;                // rx -> tick
  std::vector<ResetReq> resets;            // accept -> tick, under ready_mu
  std::vector<std::mutex> resume_mu;
  std::vector<std::vector<int>> resume;    // tick/tx -> rx: slots with a free buffer again

  std::mutex job_mu;
  std::condition_variable job_cv, job_done_cv;
  int64_t jobs_published = 0;              // job k of the run lives in jobs[k & 1] (under job_mu)

  // stats
  std::atomic<int64_t> frames_done{0}, ticks{0}, rx_bytes{0}, tx_bytes{0}, in_conns{0}, out_conns{0}, dropped{0}, numeric_resets{0},
      overruns{0}, batch_sum{0};
  std::atomic<int64_t> step_us{0};
  // stall diagnostics (printed at close when VAPX_INGEST_DEBUG is set): longest single pass of an rx thread over its ready sockets, longest gap
  // between two passes that both had work, longest step
  std::atomic<int64_t> dbg_rx_pass_us{0}, dbg_rx_gap_us{0}, dbg_step_us{0}, dbg_send_us{0}, dbg_job_tx_us{0}, dbg_recv_us{0};
  double dbg_t_in_first = 0, dbg_t_in_last = 0, dbg_t_out_first = 0, dbg_t_out_last = 0;   // accept thread only: CLOCK_MONOTONIC of the first / last adopted connection
  std::atomic<int64_t> accept_fd_errors{0};   // accept4() failed for lack of descriptors (EMFILE / ENFILE): the process limit is below 2 x streams
  Hist lat;
  std::atomic<int64_t> late10{0};          // packets of the current latency window handed over > 10 ms after their frame was complete
  bool no_lowat = false;                   // VAPX_INGEST_NO_LOWAT set at open: wake per packet as rounds 1-4 did (A/B measurements only)
  bool debug = false;                      // VAPX_INGEST_DEBUG set at open: per-call stall diagnostics (two clock reads per recv / sendmsg)
  std::string err;
  bool pinned_blocks = true;               // staging came from vapx_host_alloc (false: plain calloc, no HIP device)
  // link to a front door in ANOTHER process (vapx_ingest_attach_link): accepted connections arrive as descriptors over a unix socket,
  // slot releases / listener drops are reported back
  int link_fd = -1;
  std::mutex link_mu;                      // serialises the sends (rx / tx / link threads)
  std::thread link_thread;

  uint8_t* rawbuf(int slot, int buf) { return (uint8_t*)stage + ((size_t)slot * NBUF + buf) * frame_stride; }
  float* f32buf(int slot, int buf) { return (float*)rawbuf(slot, buf); }
  double* f64buf(int slot, int buf) { return echo.data() + ((size_t)slot * NBUF + buf) * echo_stride; }
};

namespace {

int listen_on(int port, bool any, int* bound) {
  int s = socket(AF_INET, SOCK_STREAM | SOCK_NONBLOCK, 0);
  if (s < 0) return -1;
  int one = 1;
  setsockopt(s, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
  sockaddr_in a;
  memset(&a, 0, sizeof a);
  a.sin_family = AF_INET;
  a.sin_addr.s_addr = htonl(any ? INADDR_ANY : INADDR_LOOPBACK);
  a.sin_port = htons((uint16_t)port);
  if (bind(s, (sockaddr*)&a, sizeof a) != 0 || listen(s, 8192) != 0) { close(s); return -1; }
  socklen_t len = sizeof a;
  getsockname(s, (sockaddr*)&a, &len);
  *bound = ntohs(a.sin_port);
  return s;
}

// tags in epoll_event.data.u64: low 32 bits slot (or a listen-socket / wake id), high bits kind
constexpr uint64_t K_DATA = 0, K_LISTEN_IN = 1ull << 32, K_LISTEN_OUT = 2ull << 32, K_WAKE = 3ull << 32;

void ep_add(int ep, int fd, uint64_t tag) {
  epoll_event ev;
  memset(&ev, 0, sizeof ev);
  ev.events = EPOLLIN;
  ev.data.u64 = tag;
  epoll_ctl(ep, EPOLL_CTL_ADD, fd, &ev);
}
void ep_mod(int ep, int fd, uint64_t tag, bool want_in) {
  epoll_event ev;
  memset(&ev, 0, sizeof ev);
  ev.events = want_in ? EPOLLIN : 0;
  ev.data.u64 = tag;
  epoll_ctl(ep, EPOLL_CTL_MOD, fd, &ev);
}

void kick(int efd) {
  uint64_t one = 1;
  ssize_t r = write(efd, &one, 8);
  (void)r;
}

int pick_free(Slot& s) {
  for (int b = 0; b < NBUF; ++b) {
    int expect = B_FREE;
    if (s.state[b].compare_exchange_strong(expect, B_FILLING)) return b;
  }
  return -1;
}

// free a frame buffer and, if its stream was paused for lack of buffers, ask its rx thread to resume it
void release_buf(vapx_ingest* g, int slot, int buf) {
  g->slots[slot].state[buf].store(B_FREE, std::memory_order_release);
  const int r = slot % g->R;
  bool need = false;
  {
    std::lock_guard<std::mutex> lk(g->resume_mu[r]);
    // a stale read only costs a spurious wake-up
    if (g->slots[slot].paused.load(std::memory_order_acquire)) { g->resume[r].push_back(slot); need = true; }
  }
  if (need) kick(g->wake[r]);
}

// ---- link protocol (front-door process <-> worker process), one SOCK_SEQPACKET unix socket per worker ----
struct LinkMsg { int32_t kind, a, b, c; };
enum { LK_HELLO = 1,      // worker -> door: a = dialogue slots, b = frame_hz, c = mode | broadcast << 8
       LK_ADOPT_IN = 2,   // door -> worker: a = local slot, + the accepted input socket (SCM_RIGHTS)
       LK_ADOPT_OUT = 3,  // door -> worker: a = local slot the listener attaches to (ignored by a broadcast shard), + the socket
       LK_IN_CLOSED = 4,  // worker -> door: the input connection of slot a is gone (the slot is free again)
       LK_OUT_CLOSED = 5  // worker -> door: a listener of slot a was dropped (broadcast shard: a = -1)
};

bool link_send(int link, std::mutex* mu, const LinkMsg& m, int pass_fd = -1) {
  msghdr mh;
  memset(&mh, 0, sizeof mh);
  iovec iov{(void*)&m, sizeof m};
  mh.msg_iov = &iov; mh.msg_iovlen = 1;
  alignas(cmsghdr) char ctl[CMSG_SPACE(sizeof(int))];
  if (pass_fd >= 0) {
    memset(ctl, 0, sizeof ctl);
    mh.msg_control = ctl; mh.msg_controllen = sizeof ctl;
    cmsghdr* c = CMSG_FIRSTHDR(&mh);
    c->cmsg_level = SOL_SOCKET; c->cmsg_type = SCM_RIGHTS; c->cmsg_len = CMSG_LEN(sizeof(int));
    memcpy(CMSG_DATA(c), &pass_fd, sizeof(int));
  }
  std::unique_lock<std::mutex> lk;
  if (mu) lk = std::unique_lock<std::mutex>(*mu);
  for (;;) {
    ssize_t w = sendmsg(link, &mh, MSG_NOSIGNAL);
    if (w == (ssize_t)sizeof m) return true;
    if (w < 0 && (errno == EINTR)) continue;
    if (w < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) { pollfd p{link, POLLOUT, 0}; poll(&p, 1, 50); continue; }
    return false;
  }
}

// one message (and at most one descriptor); returns 1, 0 = nothing within `timeout_ms`, -1 = the peer is gone
int link_recv(int link, LinkMsg* m, int* got_fd, int timeout_ms) {
  pollfd p{link, POLLIN, 0};
  const int pr = poll(&p, 1, timeout_ms);
  if (pr == 0) return 0;
  if (pr < 0) return errno == EINTR ? 0 : -1;
  msghdr mh;
  memset(&mh, 0, sizeof mh);
  iovec iov{m, sizeof *m};
  mh.msg_iov = &iov; mh.msg_iovlen = 1;
  alignas(cmsghdr) char ctl[CMSG_SPACE(sizeof(int))];
  mh.msg_control = ctl; mh.msg_controllen = sizeof ctl;
  ssize_t r = recvmsg(link, &mh, MSG_CMSG_CLOEXEC | MSG_DONTWAIT);
  if (r < 0) return (errno == EAGAIN || errno == EWOULDBLOCK || errno == EINTR) ? 0 : -1;
  if (r == 0) return -1;
  if (got_fd) {
    *got_fd = -1;
    for (cmsghdr* c = CMSG_FIRSTHDR(&mh); c; c = CMSG_NXTHDR(&mh, c))
      if (c->cmsg_level == SOL_SOCKET && c->cmsg_type == SCM_RIGHTS) memcpy(got_fd, CMSG_DATA(c), sizeof(int));
  }
  return r == (ssize_t)sizeof *m ? 1 : -1;
}

void link_event(vapx_ingest* g, int kind, int slot) {
  if (g->link_fd >= 0) link_send(g->link_fd, &g->link_mu, LinkMsg{kind, slot, 0, 0});
}

void drop_input(vapx_ingest* g, int r, int slot) {
  Slot& s = g->slots[slot];
  if (s.fd_in < 0) return;
  epoll_ctl(g->ep[r], EPOLL_CTL_DEL, s.fd_in, nullptr);
  close(s.fd_in);
  if (s.wbuf >= 0) { s.state[s.wbuf].store(B_FREE); s.wbuf = -1; }
  s.fill = 0; s.backlog.clear(); s.paused = false;
  {
    std::lock_guard<std::mutex> lk(g->slots_mu);
    s.fd_in = -1;
    if (slot < g->free_hint) g->free_hint = slot;
    s.gen.fetch_add(1);                     // frames of this connection still queued are dropped by the tick thread
  }
  link_event(g, LK_IN_CLOSED, slot);       // (before the counter: who sees the count drop finds the door's mirror told already)
  g->in_conns.fetch_sub(1);
}

// the slot's write buffer holds a whole frame: hand it to the tick thread
void frame_complete(vapx_ingest* g, int slot, Slot& s) {
  const int b = s.wbuf;
  const double t = mono_now();
  s.t_ready[b] = t;
  if (s.dbg_ready.fetch_add(1, std::memory_order_relaxed) == 0) s.dbg_t_first_ready = t;
  s.state[b].store(B_READY, std::memory_order_release);
  s.wbuf = -1; s.fill = 0;
  {
    std::lock_guard<std::mutex> lk(g->ready_mu);
    g->ready.push_back({slot, b, s.gen.load(std::memory_order_relaxed), t, s.cls, s.cls2});
  }
  g->ready_cv.notify_one();
}

// a channel's row of a raw format as the result packet echoes it: the decoded samples as float64, [hop]
void expand_raw(const InGeo& q, const uint8_t* raw, double* e) {
  const size_t n = (size_t)q.hop;
  if (q.fmt == VAPX_PCM_S16) {
    for (size_t i = 0; i < n; ++i) { int16_t v; memcpy(&v, raw + 2 * i, 2); e[i] = (double)v * 0x1p-15; }
  } else {
    const int16_t* t = q.fmt == VAPX_PCM_MULAW ? kMulaw : kAlaw;
    for (size_t i = 0; i < n; ++i) e[i] = (double)t[raw[i]] * 0x1p-15;
  }
}

// wire bytes of a whole frame of the slot's connection: both channels' samples, interleaved or in planar packets
size_t frame_wire_bytes(const vapx_ingest* g, const Slot& s) { return g->geo[s.cls].wire_row() + g->geo[s.cls2].wire_row(); }

// The f64 move, the only one: `n` groups of CH consecutive f64 samples (2: interleaved pairs, 1: a run of one channel) -> sample c of group
// i goes to the f64 echo d[c][i] and, cast, to the f32 staging f[c][i].  The gain is a float64 multiply BEFORE the f32 cast
// (vap_main.py:393-395); without one the cast is torch.tensor(float64).float() (vap_main.py:266-270)
template <int CH, bool GAIN>
inline void move_f64_run(const uint8_t* src, size_t n, double gain, double* const* d, float* const* f) {
  for (size_t i = 0; i < n; ++i) {
    double v[CH];
    memcpy(v, src + i * 8 * CH, 8 * CH);
    for (int c = 0; c < CH; ++c) {
      const double a = GAIN ? v[c] * gain : v[c];
      d[c][i] = a; f[c][i] = (float)a;
    }
  }
}
template <int CH>
inline void move_f64(const uint8_t* src, size_t n, double gain, double* const* d, float* const* f) {
  if (gain != 1.0) move_f64_run<CH, true>(src, n, gain, d, f);
  else move_f64_run<CH, false>(src, n, gain, d, f);
}

// f64 samples of a frame buffer: `at` = wire bytes of this run (a frame's interleaved pairs, or one channel's part of a planar frame) already
// taken, `room` = wire bytes to the end of the run, d / f = where the run's first group goes.  A group split across two reads waits in
// s.partial.  Returns the bytes taken from p[0, n)
template <int CH>
size_t take_f64(Slot& s, size_t at, size_t room, const uint8_t* p, size_t n, double gain, double* const* d0, float* const* f0) {
  constexpr size_t U = 8 * CH;
  const size_t i0 = at / U, held = at % U;
  double* d[CH]; float* f[CH];
  for (int c = 0; c < CH; ++c) { d[c] = d0[c] + i0; f[c] = f0[c] + i0; }
  if (held || n < U) {                      // finish (or begin) a group split across two reads
    const size_t take = std::min(U - held, n);
    memcpy(s.partial + held, p, take);
    if (held + take == U) move_f64<CH>(s.partial, 1, gain, d, f);
    return take;
  }
  const size_t groups = std::min(room, n) / U;
  move_f64<CH>(p, groups, gain, d, f);
  return groups * U;
}

// raw interleaved (ch1, ch2) samples of bps bytes are de-interleaved into the two rows of the staging `d` as they are: no cast, no f32
// staging, no f64 echo copy.  `at` = wire bytes of the frame already taken; a pair split across two reads is placed byte by byte
size_t take_raw_pairs(uint8_t* d, size_t hop, size_t bps, size_t at, const uint8_t* p, size_t n) {
  const size_t pb = 2 * bps, i0 = at / pb, o = at % pb;
  if (o || n < pb) {
    const size_t take = std::min(pb - o, n);
    for (size_t k = 0; k < take; ++k) d[(((o + k) / bps) * hop + i0) * bps + (o + k) % bps] = p[k];
    return take;
  }
  const size_t pairs = std::min(n / pb, hop - i0);
  if (bps == 2) {
    uint8_t *d1 = d + i0 * 2, *d2 = d + (hop + i0) * 2;
    for (size_t i = 0; i < pairs; ++i) { memcpy(d1 + 2 * i, p + 4 * i, 2); memcpy(d2 + 2 * i, p + 4 * i + 2, 2); }
  } else {
    uint8_t *d1 = d + i0, *d2 = d + hop + i0;
    for (size_t i = 0; i < pairs; ++i) { d1[i] = p[2 * i]; d2[i] = p[2 * i + 1]; }
  }
  return pairs * pb;
}

// Decode `n` bytes of the stream into the slot's frame buffers; returns bytes consumed (< n: no free buffer).  The frame buffer, the
// position in the frame (s.fill, in wire bytes for every kind of connection) and the hand-over of a complete frame are here; what differs
// is the framing - interleaved (ch1, ch2) pairs, or a pair port's planar 10 ms packets: channel 1's samples in its class's wire form, then
// channel 2's in its own - and the move of a run of samples: f64 (take_f64), or raw bytes as they are
size_t feed(vapx_ingest* g, int slot, const uint8_t* p, size_t n) {
  Slot& s = g->slots[slot];
  const InGeo* q[2] = {&g->geo[s.cls], &g->geo[s.cls2]};
  const size_t total = frame_wire_bytes(g, s), hop = (size_t)q[0]->hop;
  const double gain = g->cfg.gain;
  size_t used = 0;
  while (used < n) {
    if (s.wbuf < 0) {
      s.wbuf = pick_free(s);
      if (s.wbuf < 0) return used;          // engine is two frames behind this sender
      s.fill = 0;
    }
    uint8_t* st = g->rawbuf(slot, s.wbuf);
    double* e = g->f64buf(slot, s.wbuf);
    const uint8_t* src = p + used;
    const size_t at = (size_t)s.fill, left = n - used;
    size_t took;
    if (!s.planar) {
      if (q[0]->fmt) took = take_raw_pairs(st, hop, (size_t)q[0]->bps(), at, src, left);
      else {
        double* d[2] = {e, e + hop};
        float* f[2] = {(float*)st, (float*)st + hop};
        took = take_f64<2>(s, at, total - at, src, left, gain, d, f);
      }
    } else {
      const size_t pk = (size_t)(100 / g->hz);                                 // packets per frame, and a channel's bytes of a packet
      const size_t seg[2] = {q[0]->wire_row() / pk, q[1]->wire_row() / pk}, pkt = seg[0] + seg[1];
      const size_t k = at / pkt, in_pkt = at % pkt;
      const int c = in_pkt >= seg[0];
      const size_t in_seg = in_pkt - (c ? seg[0] : 0), room = seg[c] - in_seg;   // wire bytes to the end of this channel's part of the packet
      uint8_t* row = st + (c ? q[0]->row_bytes() : 0);
      if (q[c]->fmt) {                                                         // raw: bytes as they are (a split s16 sample is just two copies)
        took = std::min(room, left);
        memcpy(row + k * seg[c] + in_seg, src, took);
      } else {
        double* d[1] = {e + (c ? g->echo_ch2(s.cls, s.cls2) : 0)};
        float* f[1] = {(float*)row};
        took = take_f64<1>(s, k * seg[c] + in_seg, room, src, left, gain, d, f);
      }
    }
    used += took; s.fill += (int)took;
    if ((size_t)s.fill == total) frame_complete(g, slot, s);   // -> tick thread
  }
  return used;
}

// Wake this socket's receive thread when the REST OF THE CURRENT FRAME is there, not for every 10 ms packet of it (SO_RCVLOWAT; epoll
// honours it): a client sends hop / 160 packets per frame (vap_main.py:373-391) and nothing can be done with a part of a frame, so 4096
// dialogues cost 82 k wake-ups + recv() calls per second instead of 410 k.  Less time on the host's cores is less exposure to whoever else
// runs there (round 5: on a box with load average 60 from other tenants every front-end thread was losing ~10 ms slices).  Re-armed only
// when the value changes: a sender that delivers whole frames never causes a setsockopt.
void arm_lowat(vapx_ingest* g, Slot& s) {
  long need = (long)frame_wire_bytes(g, s) - (s.wbuf >= 0 ? s.fill : 0);
  if (need < 1) need = 1;
  if (need > 65536) need = 65536;           // (5 Hz frames are 51 KB; stay well inside the receive buffer)
  if ((int)need == s.lowat || s.fd_in < 0 || g->no_lowat) return;
  int v = (int)need;
  if (setsockopt(s.fd_in, SOL_SOCKET, SO_RCVLOWAT, &v, sizeof v) == 0) s.lowat = v;
}

void on_data(vapx_ingest* g, int r, int slot, uint8_t* scratch, size_t cap, uint32_t events) {
  Slot& s = g->slots[slot];
  if (s.fd_in < 0) return;
  if (s.paused) {
    // a paused slot is armed with events = 0, but EPOLLHUP / EPOLLERR are reported regardless (level-triggered): never read
    // new bytes past the parked backlog (they would overtake it), and a peer that is gone is dropped instead of spinning here
    if (events & (EPOLLHUP | EPOLLERR)) drop_input(g, r, slot);
    return;
  }
  for (int round = 0; round < 4; ++round) {   // bounded work per wake-up: fairness between streams
    const double tr0 = g->debug ? mono_now() : 0.0;
    ssize_t n = recv(s.fd_in, scratch, cap, 0);
    if (g->debug) atomic_max(g->dbg_recv_us, (int64_t)((mono_now() - tr0) * 1e6));   // longest recv() call
    if (n < 0) {
      if (errno == EAGAIN || errno == EWOULDBLOCK || errno == EINTR) { arm_lowat(g, s); return; }
      drop_input(g, r, slot);
      return;
    }
    if (n == 0) { drop_input(g, r, slot); return; }
    g->rx_bytes.fetch_add(n, std::memory_order_relaxed);
    size_t used = feed(g, slot, scratch, (size_t)n);
    if (used < (size_t)n) {                 // no free frame buffer: park the rest and stop reading this socket
      s.backlog.insert(s.backlog.end(), scratch + used, scratch + n);   // (append: never overwrite bytes parked earlier)
      {
        std::lock_guard<std::mutex> lk(g->resume_mu[r]);
        s.paused = true;
      }
      g->overruns.fetch_add(1);
      ep_mod(g->ep[r], s.fd_in, K_DATA | (uint32_t)slot, false);   // (SO_RCVLOWAT is re-armed by do_resume, from the state the backlog leaves)
      // a buffer may have been released between pick_free and `paused = true`
      for (int b = 0; b < NBUF; ++b)
        if (s.state[b].load() == B_FREE) {
          std::lock_guard<std::mutex> lk(g->resume_mu[r]);
          g->resume[r].push_back(slot);
          kick(g->wake[r]);
          break;
        }
      return;
    }
    if ((size_t)n < cap) { arm_lowat(g, s); return; }
  }
  arm_lowat(g, s);
}

void do_resume(vapx_ingest* g, int r, int slot) {
  Slot& s = g->slots[slot];
  if (s.fd_in < 0 || !s.paused) return;
  if (!s.backlog.empty()) {
    std::vector<uint8_t> b;
    b.swap(s.backlog);
    size_t used = feed(g, slot, b.data(), b.size());
    if (used < b.size()) { s.backlog.assign(b.begin() + used, b.end()); return; }   // still no buffer: stay paused
  }
  {
    std::lock_guard<std::mutex> lk(g->resume_mu[r]);
    s.paused = false;
  }
  // The backlog moved `fill`: the socket's SO_RCVLOWAT still holds what the frame open BEFORE the pause lacked, and the rest
  // of the frame open NOW may be fewer bytes than that - they would sit in the socket unread (a finite stream lost its last frame, a
  // live one got it a frame period late).  Set the threshold first, then re-enable EPOLLIN: EPOLL_CTL_MOD polls the socket against it.
  arm_lowat(g, s);
  ep_mod(g->ep[r], s.fd_in, K_DATA | (uint32_t)slot, true);
}

// accept4 failed: out of descriptors -> count it and back off (the listen socket stays readable, the level-triggered epoll would spin)
bool accept_failed_for_fds(vapx_ingest* g) {
  if (errno != EMFILE && errno != ENFILE && errno != ENOBUFS && errno != ENOMEM) return false;
  if (g->accept_fd_errors.fetch_add(1) == 0)
    fprintf(stderr, "[vapx ingest] accept: out of file descriptors (%s) - raise `ulimit -n` above 2 x streams + 64; connections wait in the listen queue\n", strerror(errno));
  std::this_thread::sleep_for(std::chrono::milliseconds(10));
  return true;
}

// lowest free input slot, or -1 (the front door compares this across shards)
int lowest_free_slot(vapx_ingest* g) {
  std::lock_guard<std::mutex> lk(g->slots_mu);
  for (int i = g->free_hint; i < g->S; ++i)
    if (g->slots[i].fd_in < 0) { g->free_hint = i; return i; }
  g->free_hint = g->S;
  return -1;
}

// Take over an accepted input connection that came in on input port `via`: the lowest free stream slot gets it, or, `at` >= 0, the slot a
// front door in another process names (its mirror of this shard is the allocator).  false = no slot for it (fd untouched)
bool adopt_in(vapx_ingest* g, int fd, int via = 0, int at = -1) {
  int slot = at;
  {
    // (round 4: this was a scan from slot 0 — 4096 dialogues connecting at once cost the accept thread ~S^2 / 2 slot visits, the output
    // connections queued behind them were attached after the first frames had been answered, and those answers went to nobody)
    std::lock_guard<std::mutex> lk(g->slots_mu);
    if (at < 0) {
      for (int i = g->free_hint; i < g->S && slot < 0; ++i)
        if (g->slots[i].fd_in < 0) slot = i;
      g->free_hint = slot >= 0 ? slot + 1 : g->S;
    } else if (at >= g->S || g->slots[at].fd_in >= 0) slot = -1;
    if (slot >= 0) g->slots[slot].fd_in = fd;
  }
  if (slot < 0) return false;
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
  const InPort& ip = g->in_ports[via];
  Slot& s = g->slots[slot];
  s.wbuf = -1; s.fill = 0; s.backlog.clear(); s.paused = false; s.lowat = 0;
  // frames of the slot's previous connection that are still queued or being sent carry their own classes (Ready::cls)
  s.cls = ip.cls; s.cls2 = ip.cls2; s.planar = ip.planar;
  {
    // the carry restarts from zeros for every connection (vap_main.py:368-369); reset_on_connect also clears the
    // model state, which the reference keeps.  Applied by the tick thread before its next step.
    std::lock_guard<std::mutex> lk(g->ready_mu);
    g->resets.push_back({slot, g->cfg.reset_on_connect ? 0 : 1, g->cls_table ? ip.cls : -1, ip.cls2});   // with a table: the tick thread tells the engine the stream's classes first
  }
  g->in_conns.fetch_add(1);
  if (at < 0) { const double t = mono_now(); if (g->dbg_t_in_first == 0) g->dbg_t_in_first = t; g->dbg_t_in_last = t; }   // (the accept thread's stamps: VAPX_INGEST_DEBUG)
  ep_add(g->ep[slot % g->R], fd, K_DATA | (uint32_t)slot);
  return true;
}

// input port `via` became readable
void accept_in(vapx_ingest* g, int via) {
  for (;;) {
    int fd = accept4(g->in_ports[via].lsock, nullptr, nullptr, SOCK_NONBLOCK);
    if (fd < 0) { accept_failed_for_fds(g); return; }
    if (!adopt_in(g, fd, via)) close(fd);   // every stream slot is taken
  }
}

// the (listener count, slot) an output connection attached now would get: fewest listeners, lowest index first
// (amortised O(1): a cursor walks the slots that still have `lmin` listeners and wraps with lmin + 1)
std::pair<int, int> next_listener_slot(vapx_ingest* g, int m = 0) {
  std::lock_guard<std::mutex> lk(g->slots_mu);
  OutPort& o = g->ports[m];
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = o.lcursor; i < g->S; ++i)
      if (o.lcount[i] == o.lmin) { o.lcursor = i; return {o.lmin, i}; }
    ++o.lmin; o.lcursor = 0;
  }
  return {o.lmin, 0};
}

// Take over an accepted output connection (non-blocking like vap_main.py:346-347): the k-th output connection hears the k-th stream,
// or, `at` >= 0, the stream a front door in another process names
void adopt_out(vapx_ingest* g, int fd, int m = 0, int at = -1) {
  OutPort& o = g->ports[m];
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
  g->out_conns.fetch_add(1);
  if (at < 0) { const double t = mono_now(); if (g->dbg_t_out_first == 0) g->dbg_t_out_first = t; g->dbg_t_out_last = t; }
  if (g->broadcast) { std::lock_guard<std::mutex> lk(g->slots_mu); o.out_all.push_back(fd); return; }
  const int slot = at >= 0 ? at : next_listener_slot(g, m).second;
  std::lock_guard<std::mutex> lk(g->slots_mu);
  if (at < 0) o.lcursor = slot + 1;
  ++o.lcount[slot];
  std::lock_guard<std::mutex> l2(g->slots[slot].lmu);
  g->slots[slot].listeners[m].push_back(fd);
  if (at < 0 && g->slots[slot].dbg_t_attach == 0) g->slots[slot].dbg_t_attach = mono_now();
}

void accept_out(vapx_ingest* g, int m) {
  for (;;) {
    int fd = accept4(g->ports[m].lsock, nullptr, nullptr, SOCK_NONBLOCK);
    if (fd < 0) { accept_failed_for_fds(g); return; }
    adopt_out(g, fd, m);
  }
}

// a dropped listener lowers its slot's count: the next output connection goes there first
void listener_dropped(vapx_ingest* g, int slot, int m = 0) {
  {
    std::lock_guard<std::mutex> lk(g->slots_mu);
    OutPort& o = g->ports[m];
    if (--o.lcount[slot] < o.lmin) { o.lmin = o.lcount[slot]; o.lcursor = slot; }
    else if (o.lcount[slot] == o.lmin && slot < o.lcursor) o.lcursor = slot;
  }
  link_event(g, LK_OUT_CLOSED, slot);
}

// a descriptor that arrived over the link is whatever the door's accept made it: the receive and sender threads need it non-blocking
void set_nonblocking(int fd) {
  const int fl = fcntl(fd, F_GETFL, 0);
  if (fl >= 0) fcntl(fd, F_SETFL, fl | O_NONBLOCK);
}

void link_main(vapx_ingest* g) {
  while (!g->stop.load()) {
    LinkMsg m;
    int fd = -1;
    const int rc = link_recv(g->link_fd, &m, &fd, 100);
    if (rc == 0) continue;
    if (rc < 0) break;                       // the front door is gone: keep serving the dialogues we have, take no new ones
    if (fd >= 0 && (m.kind == LK_ADOPT_IN || m.kind == LK_ADOPT_OUT)) set_nonblocking(fd);
    if (m.kind == LK_ADOPT_IN) {
      if (fd >= 0 && (m.a < 0 || !adopt_in(g, fd, 0, m.a))) { close(fd); link_event(g, LK_IN_CLOSED, m.a); }   // (cannot happen while the door's mirror is right)
    } else if (m.kind == LK_ADOPT_OUT) {
      if (fd >= 0) adopt_out(g, fd, 0, m.a >= 0 && m.a < g->S ? m.a : 0);
    } else if (fd >= 0) close(fd);
  }
}

void accept_main(vapx_ingest* g) {
  epoll_event evs[8];
  while (!g->stop.load()) {
    int n = epoll_wait(g->ep_accept, evs, 8, 100);
    for (int i = 0; i < n; ++i) {
      const uint64_t kind = evs[i].data.u64 & ~0xffffffffull;
      if (kind == K_LISTEN_IN) accept_in(g, (int)(evs[i].data.u64 & 0xffffffffu));
      else if (kind == K_LISTEN_OUT) accept_out(g, (int)(evs[i].data.u64 & 0xffffffffu));
    }
  }
}


void rx_main(vapx_ingest* g, int r) {
  std::vector<uint8_t> scratch(256 * 1024);
  epoll_event evs[256];
  double t_last_busy = 0.0;
  while (!g->stop.load()) {
    int n = epoll_wait(g->ep[r], evs, 256, 100);
    const double t_in = g->debug ? mono_now() : 0.0;
    if (g->debug && n > 0 && t_last_busy > 0.0) atomic_max(g->dbg_rx_gap_us, (int64_t)((t_in - t_last_busy) * 1e6));
    for (int i = 0; i < n; ++i) {
      const uint64_t tag = evs[i].data.u64, kind = tag & ~0xffffffffull;
      if (kind == K_WAKE) {
        uint64_t v;
        ssize_t rr = read(g->wake[r], &v, 8);
        (void)rr;
        std::vector<int> todo;
        {
          std::lock_guard<std::mutex> lk(g->resume_mu[r]);
          todo.swap(g->resume[r]);
        }
        for (int slot : todo) do_resume(g, r, slot);
      } else on_data(g, r, (int)(tag & 0xffffffffu), scratch.data(), scratch.size(), evs[i].events);
    }
    if (g->debug) {
      if (n > 0) {
        t_last_busy = mono_now();
        atomic_max(g->dbg_rx_pass_us, (int64_t)((t_last_busy - t_in) * 1e6));
      } else t_last_busy = 0.0;
    }
  }
}

// send one result packet to one listener; false = the listener could not take it (caller drops it)
bool send_packet(int fd, iovec* iov, int niov, size_t total) {
  msghdr mh;
  memset(&mh, 0, sizeof mh);
  mh.msg_iov = iov;
  mh.msg_iovlen = niov;
  ssize_t n = sendmsg(fd, &mh, MSG_NOSIGNAL | MSG_DONTWAIT);
  return n == (ssize_t)total;
}

void tx_main(vapx_ingest* g, int x) {
  std::vector<uint8_t> tail(64 + 8 * 256);
  size_t raw_hop = 0;
  for (int c = 0; c < g->n_cls; ++c)
    if (g->geo[c].fmt) raw_hop = std::max(raw_hop, (size_t)g->geo[c].hop);
  std::vector<double> expanded(2 * raw_hop);   // a raw format: the echo of a row's channels, decoded from the staging by the table
  constexpr int MAX_R = 10;                  // 50 Hz -> 5 Hz
  int64_t next = 0;                          // the job this thread sends next: every sender walks over EVERY job, in publication order
  while (true) {
    // Per-stream order without serialising the ticks: the rows of a job are partitioned by slot % X, so a stream's packets always leave
    // through the same thread, and that thread works through the jobs in the order they were published — a listener can never see frame
    // k + 1 before frame k (round 4 kept the order by sending one job at a time: every sender idled while the last chunk of a tick was
    // still going out; advisor r04).  A job is handed back to the tick thread when all X senders are through with it.
    int j = -1;
    {
      std::unique_lock<std::mutex> lk(g->job_mu);
      g->job_cv.wait(lk, [&] { return g->jobs_published > next || g->stop.load(); });
      if (g->jobs_published <= next) return;   // stopping, nothing left to send
      j = (int)(next & 1);
    }
    Job& job = g->jobs[j];
    for (int k : job.part[x]) {
      const Ready& rd = job.rows[k];
      Slot& s = g->slots[rd.slot];
      const InGeo& q = g->geo[rd.cls];
      const InGeo* qc[2] = {&q, &g->geo[rd.cls2]};   // channel 2's class differs on a pair port's stream (M = 1, R = 1 there: check_classes)
      const int hop = q.hop;
      if (job.bad[k]) {   // the stream was reset (status 1 in some model): a slower model's frame in the making starts over with it
        for (int m = 0; m < g->M; ++m)
          if (g->ports[m].R > 1) g->ports[m].hist_n[rd.slot] = 0;
      } else {
        // u32 len | f64 t | u32 n | x1 | u32 n | x2 | tail   (util.py:122-143; length prefix vap_main.py:446-448); a trunk group sends one
        // packet per model, each to its own port's listeners, tail in that model's framing (bc util.py:193-211, nod :213-237)
        double* ec[2];                              // the echo of channel 1 and of channel 2: [hop of its class] f64
        for (int c = 0; c < 2; ++c) {
          if (qc[c]->fmt) {
            ec[c] = expanded.data() + (size_t)c * raw_hop;
            expand_raw(*qc[c], g->rawbuf(rd.slot, rd.buf) + (c ? qc[0]->row_bytes() : 0), ec[c]);
          } else ec[c] = g->f64buf(rd.slot, rd.buf) + (c ? g->echo_ch2(rd.cls, rd.cls2) : 0);
        }
        double* e = ec[0];                          // (R > 1: one class, [2][hop] contiguous in either case)
        for (int m = 0; m < g->M; ++m) {
          OutPort& o = g->ports[m];
          const float* row = job.out + (size_t)job.n * o.off + (size_t)k * o.wf;
          uint8_t head[16], mid[4];
          // a model at 1/R of the leader's rate answers every R-th leader hop of a dialogue with ONE packet echoing all R hops, what
          // its reference program sends (n = R * hop samples per channel); the hops in between (VAPX_STATUS_NO_FRAME) only add to its
          // echo history: no packet, no reset
          int held = 0;
          double* hb = nullptr;
          if (o.R > 1) {
            hb = o.hist.data() + (size_t)rd.slot * (o.R - 1) * 2 * hop;
            int& hn = o.hist_n[rd.slot];
            if (o.hist_gen[rd.slot] != rd.gen) { hn = 0; o.hist_gen[rd.slot] = rd.gen; }
            if (row[VAPX_OUT_STATUS] == (float)VAPX_STATUS_NO_FRAME) {
              if (hn < o.R - 1) { memcpy(hb + (size_t)hn * 2 * hop, e, (size_t)2 * hop * 8); ++hn; }
              continue;
            }
            held = hn;
            hn = 0;
            // a connection that began in the middle of this model's frame (carry-only reconnect: the engine's phase runs on) has no
            // samples to echo for the frame's head: that one frame goes unanswered
            if (held != o.R - 1) continue;
          }
          const uint32_t ns = (uint32_t)(hop * o.R), ns2 = (uint32_t)(qc[1]->hop * o.R);
          const int tb = encode_tail(o.mode, row, tail.data(), std::min(256, o.wf - VAPX_OUT_LOGITS));
          const uint32_t plen = 8 + (4 + 8 * ns) + (4 + 8 * ns2) + (uint32_t)tb;
          uint8_t* p = head;
          put_u32(p, plen); put_f64(p, job.t_unix); put_u32(p, ns);
          p = mid; put_u32(p, ns2);
          iovec iov[2 * MAX_R + 3];
          int niov = 0;
          iov[niov++] = {head, 16};
          for (int c = 0; c < 2; ++c) {
            if (c) iov[niov++] = {mid, 4};
            for (int q = 0; q < held; ++q) iov[niov++] = {hb + ((size_t)q * 2 + c) * hop, (size_t)hop * 8};
            iov[niov++] = {ec[c], (size_t)qc[c]->hop * 8};
          }
          iov[niov++] = {tail.data(), (size_t)tb};
          const size_t total = 4 + plen;
          auto send_to = [&](std::vector<int>& fds) {
            for (size_t i = 0; i < fds.size();) {
              const double ts0 = g->debug ? mono_now() : 0.0;
              const bool sent = send_packet(fds[i], iov, niov, total);
              if (g->debug) atomic_max(g->dbg_send_us, (int64_t)((mono_now() - ts0) * 1e6));   // longest sendmsg() call (the socket is non-blocking)
              if (sent) { g->tx_bytes.fetch_add((int64_t)total, std::memory_order_relaxed); ++i; }
              else { close(fds[i]); fds.erase(fds.begin() + i); g->dropped.fetch_add(1); g->out_conns.fetch_sub(1); if (g->broadcast) link_event(g, LK_OUT_CLOSED, -1); }
            }
          };
          if (g->broadcast) { std::lock_guard<std::mutex> lk(g->slots_mu); send_to(o.out_all); }
          else {
            size_t gone = 0;
            {
              std::lock_guard<std::mutex> lk(s.lmu);
              const size_t before = s.listeners[m].size();
              if (m == 0) {
                if (before == 0) s.dbg_nolistener.fetch_add(1, std::memory_order_relaxed);
                else if (s.dbg_sent.fetch_add(1, std::memory_order_relaxed) == 0) s.dbg_t_first_sent = mono_now();
              }
              send_to(s.listeners[m]);
              gone = before - s.listeners[m].size();
            }
            for (size_t d = 0; d < gone; ++d) listener_dropped(g, rd.slot, m);   // (slots_mu is never taken under a slot's lmu here)
          }
        }
        const double lat = mono_now() - rd.t;   // once per stream-frame: the last model's packets are with the kernel
        g->lat.add(lat);
        if (lat > 0.010) g->late10.fetch_add(1, std::memory_order_relaxed);
      }
      release_buf(g, rd.slot, rd.buf);
    }
    ++next;
    {
      std::lock_guard<std::mutex> lk(g->job_mu);
      if (++job.senders_done >= g->X) {      // every packet of this tick is out: the Job may be reused
        if (g->debug) atomic_max(g->dbg_job_tx_us, (int64_t)((unix_now() - job.t_unix) * 1e6));   // results ready -> last packet of the tick handed to the kernel
        job.busy = false;
        g->job_done_cv.notify_all();
      }
    }
  }
}

void tick_main(vapx_ingest* g) {
  std::deque<Ready> pending;
  std::vector<uint8_t> in_batch(g->S, 0);
  double first_ready = 0.0;
  int jsel = 0;
  const double max_wait = (g->cfg.max_wait_us > 0 ? g->cfg.max_wait_us : 2000) * 1e-6;
  const double util = (g->cfg.target_util_pct > 0 ? std::min(g->cfg.target_util_pct, 100) : 90) * 0.01;   // 90: measured best at the edge (6144 streams: client p99 12.6 ms vs 19.0 at 75, 16.0 unpaced)
  double earliest_next = 0.0;              // pacing: previous tick's start + its duration / util
  while (!g->stop.load()) {
    std::vector<Ready> fresh;
    std::vector<ResetReq> resets;
    {
      std::unique_lock<std::mutex> lk(g->ready_mu);
      if (g->ready.empty() && g->resets.empty()) {
        if (pending.empty()) cv_wait_for(g->ready_cv, lk, std::chrono::milliseconds(20));
        else {
          const double left = first_ready + max_wait - mono_now();
          if (left > 0) cv_wait_for(g->ready_cv, lk, std::chrono::microseconds((long)(left * 1e6) + 1));
        }
      }
      fresh.swap(g->ready);
      resets.swap(g->resets);
    }
    for (auto& rs : resets) {
      if (rs.cls >= 0) {   // a connection on a class or pair port: the stream is of those classes from its first frame on
        g->tick_cls[(size_t)2 * rs.slot] = rs.cls;
        g->tick_cls[(size_t)2 * rs.slot + 1] = rs.cls2;
        if (g->set_class) g->set_class(g->user, rs.slot, rs.cls, rs.cls2);
      }
      if (g->reset) g->reset(g->user, rs.carry_only ? -(rs.slot + 1) : rs.slot);   // negative = carry only
    }
    for (auto& rd : fresh) {
      if (rd.gen != g->slots[rd.slot].gen.load(std::memory_order_acquire)) { release_buf(g, rd.slot, rd.buf); continue; }   // connection already gone
      if (pending.empty()) first_ready = rd.t;
      pending.push_back(rd);
    }
    if (pending.empty()) continue;
    const int connected = (int)g->in_conns.load();
    int want = g->cfg.min_batch > 0 ? g->cfg.min_batch : connected;
    want = std::max(1, std::min(want, std::min(connected > 0 ? connected : 1, g->max_batch)));
    const double now = mono_now();
    if ((int)pending.size() < want && now - first_ready < max_wait) continue;
    // pacing: let the batch grow instead of the queue — but never hold a frame longer than max_wait for it (under overload
    // the oldest frame is already older than that and ticks run back to back)
    if (now < earliest_next && (int)pending.size() < g->max_batch && now - first_ready < max_wait) {
      std::unique_lock<std::mutex> lk(g->ready_mu);
      if (g->ready.empty()) cv_wait_for(g->ready_cv, lk, std::chrono::microseconds((long)((earliest_next - now) * 1e6) + 1));
      continue;
    }

    Job& job = g->jobs[jsel];
    {
      std::unique_lock<std::mutex> lk(g->job_mu);
      g->job_done_cv.wait(lk, [&] { return !job.busy || g->stop.load(); });
      if (g->stop.load()) break;
    }
    // one frame per stream per tick, oldest first; a second frame of the same stream waits for the next tick
    job.rows.clear();
    std::deque<Ready> later;
    while (!pending.empty()) {
      Ready rd = pending.front();
      pending.pop_front();
      if (rd.gen != g->slots[rd.slot].gen.load(std::memory_order_acquire)) { release_buf(g, rd.slot, rd.buf); continue; }
      if (in_batch[rd.slot] || (int)job.rows.size() >= g->max_batch) { later.push_back(rd); continue; }
      in_batch[rd.slot] = 1;
      g->slots[rd.slot].state[rd.buf].store(B_INFLIGHT);
      job.rows.push_back(rd);
    }
    pending.swap(later);
    if (!pending.empty()) first_ready = pending.front().t;
    const int n = (int)job.rows.size();
    if (n == 0) continue;
    size_t at = 0;   // frames of the staging, f32 or raw, back to back in batch order: with a table, the packed block of vapx.h "Input classes"
    for (int k = 0; k < n; ++k) {
      in_batch[job.rows[k].slot] = 0;
      g->batch_ids[k] = job.rows[k].slot;
      const size_t fb = g->frame_bytes(job.rows[k].cls, job.rows[k].cls2);
      memcpy((uint8_t*)g->batch_audio + at, g->rawbuf(job.rows[k].slot, job.rows[k].buf), fb);
      at += fb;
    }
    const double t0 = mono_now();
    const int rc = g->step(g->user, n, g->batch_ids.data(), g->batch_audio, job.out);
    const double t1 = mono_now();
    earliest_next = t0 + (t1 - t0) / util;
    g->step_us.fetch_add((int64_t)((t1 - t0) * 1e6));
    if (g->debug) atomic_max(g->dbg_step_us, (int64_t)((t1 - t0) * 1e6));
    g->ticks.fetch_add(1);
    g->batch_sum.fetch_add(n);
    if (rc != 0 && rc != VAPX_E_NUMERIC) {   // the step itself failed: nothing to send; free the frames and keep serving
      char buf[96];
      snprintf(buf, sizeof buf, "step failed with code %d", rc);
      g->err = buf;
      for (int k = 0; k < n; ++k) release_buf(g, job.rows[k].slot, job.rows[k].buf);
      continue;
    }
    job.bad.assign(n, 0);
    for (int k = 0; k < n; ++k) {
      for (int m = 0; m < g->M; ++m)
        if (job.out[(size_t)n * g->ports[m].off + (size_t)k * g->ports[m].wf + VAPX_OUT_STATUS] == 1.f) job.bad[k] = 1;   // (2: no frame due, no fault)
      if (job.bad[k]) {   // poisoned stream (in any model): fresh state, no packet on any port; counted once
        if (g->reset) g->reset(g->user, job.rows[k].slot);
        g->numeric_resets.fetch_add(1);
      }
    }
    g->frames_done.fetch_add(n);
    job.t_unix = unix_now();
    for (auto& pt : job.part) pt.clear();
    for (int k = 0; k < n; ++k) job.part[job.rows[k].slot % g->X].push_back(k);
    {
      std::lock_guard<std::mutex> lk(g->job_mu);
      job.n = n;
      job.senders_done = 0;
      job.busy = true;
      ++g->jobs_published;                   // this job is number jobs_published - 1 and sits in jobs[jsel]: publications alternate slots
    }
    g->job_cv.notify_all();
    jsel ^= 1;
  }
}

int engine_step(void* user, int32_t n, const int32_t* ids, const float* audio, float* out) {
  vapx_ingest* g = (vapx_ingest*)user;
  return vapx_step(g->engine, n, ids, audio, g->cls_table ? 0 : g->geo[0].hop, out, VAPX_AUDIO_HOST | VAPX_OUT_HOST, nullptr);   // a table: the classes size the slots
}
void engine_set_class(void* user, int32_t sid, int32_t cls, int32_t cls2) {
  vapx_ingest* g = (vapx_ingest*)user;
  if (cls != cls2) {
    if (vapx_set_stream_channel_classes) (void)vapx_set_stream_channel_classes(g->engine, sid, cls, cls2);
  } else if (vapx_set_stream_class) (void)vapx_set_stream_class(g->engine, sid, cls);
}
void engine_reset(void* user, int32_t sid) {
  vapx_ingest* g = (vapx_ingest*)user;
  if (sid < 0) (void)vapx_reset_carry(g->engine, -sid - 1);
  else (void)vapx_reset_stream(g->engine, sid);
}

// pin a thread to one core of the configured range (vapx_ingest_config.cpu_first / cpu_count); failures are ignored: placement is a
// tail-latency measure, not a correctness one
void pin_to(std::thread& t, const vapx_ingest_config& c, int k) {
  if (c.cpu_count <= 0 || !t.joinable()) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  if (c.flags & VAPX_INGEST_CORE_SET) {
    for (int i = 0; i < c.cpu_count; ++i) CPU_SET((c.cpu_first + i) % CPU_SETSIZE, &set);
  } else {
    CPU_SET((c.cpu_first + (k % c.cpu_count)) % CPU_SETSIZE, &set);
  }
  (void)pthread_setaffinity_np(t.native_handle(), sizeof set, &set);
}

// the caller's config, whatever its vintage: the struct only ever grows at the end and says how long it is
bool read_config(const vapx_ingest_config* cfg, vapx_ingest_config* out) {
  constexpr int32_t kFirst = (int32_t)offsetof(vapx_ingest_config, cpu_first);   // ABI 2 as first shipped: up to `reserved` (now `flags`)
  constexpr int32_t kPlaced = (int32_t)offsetof(vapx_ingest_config, input_format);   // ... with the thread placement, before the input format
  // ... with the input format, before the input classes: the struct then ENDED with input_format, and its tail padding is where
  // n_input_classes lives now: nothing past input_format is read from a struct of that size
  constexpr int32_t kFormatEnd = (int32_t)offsetof(vapx_ingest_config, n_input_classes);
  constexpr int32_t kFormat = (kFormatEnd + 7) & ~7;
  constexpr int32_t kClasses = (int32_t)offsetof(vapx_ingest_config, n_pair_ports);   // ... with the input classes, before the pair ports (no padding: a multiple of 8)
  static_assert(kClasses % 8 == 0, "the struct that ended with class_ports_in had no tail padding");
  if (!cfg || (cfg->struct_size != kFirst && cfg->struct_size != kPlaced && cfg->struct_size != kFormat && cfg->struct_size != kClasses &&
               cfg->struct_size != (int32_t)sizeof(vapx_ingest_config))) return false;
  memset(out, 0, sizeof *out);
  memcpy(out, cfg, cfg->struct_size == kFormat ? (size_t)kFormatEnd : (size_t)cfg->struct_size);
  out->struct_size = (int32_t)sizeof(vapx_ingest_config);
  return true;
}

thread_local std::string g_open_error;   // vapx_ingest_last_open_error
int open_refused(const char* why) { g_open_error = why; return VAPX_E_INVAL; }

// what the config's input format may be: engine_fmt is the engine's (vapx_get_input_format), or -1 for a front-end over a step function,
// which takes the config's.  VAPX_OK or the refusal, with its message
int check_format(const vapx_ingest_config* cfg, int engine_fmt) {
  if (cfg->input_format < VAPX_PCM_F32 || cfg->input_format > VAPX_PCM_ALAW)
    return open_refused("input_format: known are 0 (f64 pairs, the reference's framing), 1 (s16), 2 (mulaw) and 3 (alaw)");
  if (engine_fmt >= 0 && cfg->input_format != 0 && cfg->input_format != engine_fmt)
    return open_refused("vapx_ingest_config.input_format differs from the engine's input format (vapx_set_input_format): leave it 0 or make them equal");
  const int fmt = engine_fmt >= 0 ? engine_fmt : cfg->input_format;
  if (fmt && cfg->gain != 1.0 && cfg->gain != 0.0)
    return open_refused("gain with a raw input format: the gain is a float64 multiply in front of the f32 cast, and raw samples are never cast on the host");
  return VAPX_OK;
}

// What the engine behind a front-end says of its input (vapx_get_input_rate, _format, _classes).  Over a step function there is none to
// ask: 16 kHz, and the format and the table are the config's (fmt and n_cls stay -1)
struct EngineInput {
  int hz = 16000, fmt = -1, n_cls = -1;
  vapx_input_class tab[VAPX_MAX_INPUT_CLASSES];
};

// the class table a front-end serves: the engine's (n_engine > 0; the config's must then be empty or equal to it) or, over a step function
// (n_engine < 0), the config's.  Sets g->cls_table / n_cls / cls_pub (the pair ports stay in the config); VAPX_OK or the refusal, with its message
int check_classes(vapx_ingest* g, const vapx_ingest_config* cfg, int n_engine, const vapx_input_class* engine_tab) {
  const int nc = cfg->n_input_classes;
  if (nc < 0 || nc > VAPX_MAX_INPUT_CLASSES) return open_refused("n_input_classes: the table holds 0 (no classes) .. 16 entries");
  for (int i = 0; i < nc; ++i) {
    const vapx_input_class& c = cfg->input_classes[i];
    if (c.input_hz != 8000 && c.input_hz != 16000 && c.input_hz != 32000 && c.input_hz != 48000)
      return open_refused("input_classes: an input rate other than 8000, 16000, 32000 and 48000");
    if (c.format < VAPX_PCM_F32 || c.format > VAPX_PCM_ALAW) return open_refused("input_classes: formats are 0 (f64 pairs on the wire), 1 (s16), 2 (mulaw) and 3 (alaw)");
    for (int j = 0; j < i; ++j)
      if (cfg->input_classes[j].input_hz == c.input_hz && cfg->input_classes[j].format == c.format) return open_refused("input_classes: two equal entries");
    if (cfg->class_ports_in[i] < 0) return open_refused("class_ports_in: a class's input port must be >= 0 (0 = ephemeral)");
  }
  if (n_engine >= 0) {
    if (nc && nc != n_engine)
      return open_refused("vapx_ingest_config.input_classes differs from the engine's table (vapx_set_input_classes): leave it empty or make them equal");
    for (int i = 0; i < nc; ++i)
      if (cfg->input_classes[i].input_hz != engine_tab[i].input_hz || cfg->input_classes[i].format != engine_tab[i].format)
        return open_refused("vapx_ingest_config.input_classes differs from the engine's table (vapx_set_input_classes): leave it empty or make them equal");
  }
  const int n_tab = n_engine >= 0 ? n_engine : nc;
  g->cls_table = n_tab > 0;
  if (g->cls_table) g->n_cls = n_tab;
  for (int i = 0; i < n_tab; ++i) g->cls_pub[i] = n_engine >= 0 ? engine_tab[i] : cfg->input_classes[i];
  const int np = cfg->n_pair_ports;
  if (np < 0 || np > VAPX_MAX_PAIR_PORTS) return open_refused("n_pair_ports: 0 (no pair ports) .. 16 entries");
  if (np && !g->cls_table) return open_refused("pair_ports without input classes: a pair port names two classes of the table (vapx_set_input_classes, or input_classes here)");
  for (int i = 0; i < np; ++i) {
    if (cfg->pair_ports[i].cls_ch1 < 0 || cfg->pair_ports[i].cls_ch1 >= g->n_cls || cfg->pair_ports[i].cls_ch2 < 0 || cfg->pair_ports[i].cls_ch2 >= g->n_cls)
      return open_refused("pair_ports: a channel's class is not an index into the table of input classes");
    if (cfg->pair_ports[i].port_in < 0) return open_refused("pair_ports: a pair port's input port must be >= 0 (0 = ephemeral)");
  }
  if (!g->cls_table) return VAPX_OK;
  if (cfg->input_format) return open_refused("input_format together with input classes: the format is each class's own");
  if (cfg->port_in < 0 || cfg->port_out < 0)
    return open_refused("a front-end with input classes cannot be a passive shard (port_in = -1): the front door has one input port, a class is known by its port");
  if (g->M > 1) return open_refused("a trunk group's front-end takes no input classes: multi-port groups are not part of the class ports yet");
  if (cfg->gain != 1.0 && cfg->gain != 0.0)
    for (int i = 0; i < g->n_cls; ++i)
      if (g->cls_pub[i].format)
        return open_refused("gain with a raw input class: the gain is a float64 multiply in front of the f32 cast, and raw samples are never cast on the host");
  return VAPX_OK;
}

// The first half of every open: the config against what the engine says of its input, and the one description of the input that follows
// from the two - classes, geometries, strides, input ports.  g->S, max_batch, hz and the output ports are set.  Touches nothing outside
// *g: a refusal here leaves the engine as it was
int configure(vapx_ingest* g, const vapx_ingest_config* cfg_in, const EngineInput& e = EngineInput()) {
  if (!read_config(cfg_in, &g->cfg)) return VAPX_E_INVAL;
  const vapx_ingest_config* cfg = &g->cfg;
  g->debug = getenv("VAPX_INGEST_DEBUG") != nullptr;
  g->no_lowat = getenv("VAPX_INGEST_NO_LOWAT") != nullptr;
  { const int rc = check_classes(g, cfg, e.n_cls, e.tab); if (rc) return rc; }
  if (g->cfg.gain == 0.0) g->cfg.gain = 1.0;
  { const int rc = check_format(cfg, e.fmt); if (rc) return rc; }
  g->R = cfg->rx_threads > 0 ? std::min(cfg->rx_threads, 16) : 2;
  g->X = cfg->tx_threads > 0 ? std::min(cfg->tx_threads, 16) : 2;
  g->broadcast = cfg->broadcast < 0 ? (g->S == 1) : (cfg->broadcast != 0);
  g->n_in = 0;
  if (!g->cls_table) {   // the one-class case: the engine's rate and format (or the config's format), one input port
    g->cls_pub[0] = {e.hz, e.fmt >= 0 ? e.fmt : cfg->input_format};
    g->in_ports[g->n_in++].port = cfg->port_in;
  } else {               // one input port per class (port_in is ignored), then the pair ports
    for (int c = 0; c < g->n_cls; ++c) { InPort& ip = g->in_ports[g->n_in++]; ip.port = cfg->class_ports_in[c]; ip.cls = ip.cls2 = c; }
    for (int p = 0; p < cfg->n_pair_ports; ++p) {
      InPort& ip = g->in_ports[g->n_in++];
      ip.port = cfg->pair_ports[p].port_in; ip.cls = cfg->pair_ports[p].cls_ch1; ip.cls2 = cfg->pair_ports[p].cls_ch2; ip.planar = true;
    }
  }
  g->frame_stride = g->echo_stride = 0;
  for (int c = 0; c < g->n_cls; ++c) {
    InGeo& q = g->geo[c];
    q.fmt = g->cls_pub[c].format; q.in_hz = g->cls_pub[c].input_hz; q.hop = q.in_hz / g->hz;
    g->frame_stride = std::max(g->frame_stride, q.frame_bytes());
    if (!q.fmt) g->echo_stride = std::max(g->echo_stride, (size_t)2 * q.hop);   // a raw format keeps no f64 echo
  }
  return VAPX_OK;
}

// The second half: staging, sockets, threads
int start(vapx_ingest* g) {
  const vapx_ingest_config* cfg = &g->cfg;
  for (int m = 0; m < g->M; ++m) {
    OutPort& o = g->ports[m];
    if (o.R <= 1) continue;   // input framing, ticks and batching stay the leader's; this model's packets echo R leader hops as received
    o.hist.assign((size_t)g->S * (o.R - 1) * 2 * g->geo[0].hop, 0.0);
    o.hist_n.assign(g->S, 0);
    o.hist_gen.assign(g->S, 0u);
  }
  g->tick_cls.assign((size_t)g->S * 2, 0);
  g->slots.reset(new Slot[g->S]);
  const size_t per = ((size_t)g->S * NBUF * g->frame_stride + 3) / 4;      // the staging blocks in floats: f32 samples, or raw ones of bps bytes
  const size_t ba = ((size_t)g->max_batch * g->frame_stride + 3) / 4;
  const size_t ob = (size_t)g->max_batch * g->row_floats;
  // page-locked staging so vapx_step DMAs straight out of / into it; without a HIP device (host-logic tests over a step
  // function) plain memory does
  g->stage = (float*)vapx_host_alloc(per * sizeof(float));
  g->pinned_blocks = g->stage != nullptr;
  auto grab = [&](size_t n) { return (float*)(g->pinned_blocks ? vapx_host_alloc(n * sizeof(float)) : calloc(n, sizeof(float))); };
  if (!g->stage) g->stage = grab(per);
  if (g->echo_stride) g->echo.assign((size_t)g->S * NBUF * g->echo_stride, 0.0);
  g->batch_audio = grab(ba);
  g->batch_ids.assign(g->max_batch, 0);
  for (auto& j : g->jobs) {
    j.out = grab(ob);
    if (j.out) memset(j.out, 0, ob * sizeof(float));   // hipHostMalloc memory is not zeroed: a step function may leave columns unset
    j.rows.reserve(g->max_batch);
    j.part.assign(g->X, {});
  }
  if (!g->stage || !g->batch_audio || !g->jobs[0].out || !g->jobs[1].out) return VAPX_E_NOMEM;
  // One descriptor per input connection and one per listener: 2 x S and some.  Raise the soft RLIMIT_NOFILE towards the hard limit if it
  // is short, and say so if the hard limit is short too: connections beyond it wait in the listen queue (accept4 fails with EMFILE, counted
  // in accept_fd_errors), and a dialogue whose output connection is not attached yet loses its results — they go to nobody
  if (!(cfg->flags & VAPX_INGEST_KEEP_NOFILE)) {
    const rlim_t need = (rlim_t)2 * (rlim_t)g->S + 256;
    rlimit rl;
    if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur != RLIM_INFINITY && rl.rlim_cur < need) {
      rlimit want = rl;
      want.rlim_cur = rl.rlim_max == RLIM_INFINITY ? need : std::min<rlim_t>(rl.rlim_max, std::max<rlim_t>(need, rl.rlim_cur));
      (void)setrlimit(RLIMIT_NOFILE, &want);
      if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur < need)
        fprintf(stderr, "[vapx ingest] RLIMIT_NOFILE is %llu (hard limit), %llu are needed for %d dialogue slots with one listener each: later "
                "connections will wait in the listen queue\n", (unsigned long long)rl.rlim_cur, (unsigned long long)need, g->S);
    }
  }
  // port_in < 0: a PASSIVE shard of a multi-GPU front door (vapx_frontdoor_open): it listens on nothing, connections are handed to it
  const bool passive = cfg->port_in < 0;
  if (passive != (cfg->port_out < 0)) return VAPX_E_INVAL;   // a shard is passive on BOTH ports or on none (-1 / >= 0 mixed is a configuration error)
  if (passive) g->in_ports[0].port = 0;
  else {
    for (int i = 0; i < g->n_in; ++i) {
      InPort& ip = g->in_ports[i];
      ip.lsock = listen_on(ip.port, cfg->bind_any != 0, &ip.port);
      if (ip.lsock < 0) return VAPX_E_INVAL;
    }
    for (int m = 0; m < g->M; ++m) {
      g->ports[m].lsock = listen_on(m ? g->cfg_ports_out[m] : cfg->port_out, cfg->bind_any != 0, &g->ports[m].port);
      if (g->ports[m].lsock < 0) return VAPX_E_INVAL;
    }
  }
  g->resume_mu = std::vector<std::mutex>(g->R);
  g->resume.assign(g->R, {});
  for (int r = 0; r < g->R; ++r) {
    g->ep.push_back(epoll_create1(0));
    g->wake.push_back(eventfd(0, EFD_NONBLOCK));
    ep_add(g->ep[r], g->wake[r], K_WAKE);
  }
  for (int m = 0; m < g->M; ++m) g->ports[m].lcount.assign(g->S, 0);
  if (!passive) {
    g->ep_accept = epoll_create1(0);          // own thread: a connect storm must not starve the streams of a receive thread
    for (int i = 0; i < g->n_in; ++i) ep_add(g->ep_accept, g->in_ports[i].lsock, K_LISTEN_IN | (uint32_t)i);
    for (int m = 0; m < g->M; ++m) ep_add(g->ep_accept, g->ports[m].lsock, K_LISTEN_OUT | (uint32_t)m);
    g->accept_thread = std::thread(accept_main, g);
  }
  for (int r = 0; r < g->R; ++r) g->rx_threads.emplace_back(rx_main, g, r);
  for (int x = 0; x < g->X; ++x) g->tx_threads.emplace_back(tx_main, g, x);
  g->tick_thread = std::thread(tick_main, g);
  // placement: tick + accept on the first core of the range, then one core per receive thread, then one per sender
  pin_to(g->tick_thread, g->cfg, 0);
  pin_to(g->accept_thread, g->cfg, 0);
  for (int r = 0; r < g->R; ++r) pin_to(g->rx_threads[r], g->cfg, 1 + r);
  for (int x = 0; x < g->X; ++x) pin_to(g->tx_threads[x], g->cfg, 1 + g->R + x);
  return VAPX_OK;
}

int engine_group_step(void* user, int32_t n, const int32_t* ids, const float* audio, float* wire_out) {
  vapx_ingest* g = (vapx_ingest*)user;
  return vapx_step_group(g->engine, n, ids, audio, g->geo[0].hop, wire_out, VAPX_AUDIO_HOST | VAPX_OUT_HOST, nullptr);
}

// what the engine says of its input: 16 kHz, fp32 and no table unless vapx_set_input_rate / _format / _classes said otherwise (or the
// program has no such call: the weak symbols above)
EngineInput engine_input(vapx_handle engine) {
  EngineInput e;
  const int32_t hz = vapx_get_input_rate ? vapx_get_input_rate(engine) : 16000;
  const int32_t fmt = vapx_get_input_format ? vapx_get_input_format(engine) : VAPX_PCM_F32;
  const int32_t n = vapx_get_input_classes ? vapx_get_input_classes(engine, e.tab, VAPX_MAX_INPUT_CLASSES) : 0;
  e.hz = hz > 0 ? hz : 16000; e.fmt = fmt > 0 ? fmt : VAPX_PCM_F32; e.n_cls = n > 0 ? n : 0;
  return e;
}

// silence in a raw format, for the warm-up: the code of the smallest magnitude (0.0 for s16 and mulaw, 8 * 2^-15 for alaw)
int silence_byte(int fmt) { return fmt == VAPX_PCM_MULAW ? 0xFF : fmt == VAPX_PCM_ALAW ? 0xD5 : 0; }

// Warm the engine up before the first client connects: the first step of a process loads the code objects and sizes the runtime's pools
// (hundreds of ms) - paid here, `ticks` times `step` (vapx_step, or vapx_step_group: the whole group per tick) on max_batch slots of silence
// in class 0's geometry, rows of `out_floats`; then every touched stream is reset (a leader cascades).  Skipped under
// VAPX_INGEST_KEEP_STATE: the streams hold imported state and the caller has warmed the engine up before importing.  With a table every
// stream is of class 0 still and the classes size the slots (samples_per_ch = 0)
void warm_up(const vapx_ingest* g, decltype(&vapx_step) step, size_t out_floats, int ticks) {
  if (g->cfg.flags & VAPX_INGEST_KEEP_STATE) return;
  const InGeo& q = g->geo[0];
  const size_t nw = (size_t)g->max_batch;
  float* a = (float*)vapx_host_alloc(nw * q.frame_bytes());
  float* o = (float*)vapx_host_alloc(nw * out_floats * sizeof(float));
  if (a && o) {
    memset(a, silence_byte(q.fmt), nw * q.frame_bytes());
    for (int k = 0; k < ticks; ++k) (void)step(g->engine, (int32_t)nw, nullptr, a, g->cls_table ? 0 : q.hop, o, VAPX_AUDIO_HOST | VAPX_OUT_HOST, nullptr);
    for (size_t i = 0; i < nw; ++i) (void)vapx_reset_stream(g->engine, (int32_t)i);
  }
  vapx_host_free(a);
  vapx_host_free(o);
}

bool known_frame_hz(int hz) { return hz == 5 || hz == 10 || hz == 20 || hz == 50; }

// a trunk group's ports: model m's framing, the geometry of its rows in the tick's wire block (vapx_step_group) and its requested port
int setup_group(vapx_ingest* g, const int32_t* frame_hzs, const int32_t* ctx_frames, const int32_t* modes, int n_models,
                const vapx_ingest_config& cfg, const int32_t* follower_ports_out) {
  if (n_models < 1 || n_models > MAX_MODELS) return open_refused("a group serves one to three models");
  for (int m = 0; m < n_models; ++m) {
    const int hz = frame_hzs[m];
    if (!known_frame_hz(hz)) return open_refused("frame_hz must be 5, 10, 20 or 50");
    if (hz > frame_hzs[0]) return open_refused("model 0 leads the group and must be its fastest model: a follower's frame_hz exceeds it");
    if (frame_hzs[0] % hz) return open_refused("the leader's frame_hz must be an integer multiple of every follower's");
  }
  if (cfg.port_in < 0 || cfg.port_out < 0)
    return open_refused("a trunk group cannot be a passive shard (port_in = -1): the front door is single-model");
  size_t acc = 0;
  for (int m = 0; m < n_models; ++m) {
    const int wf = vapx_wire_floats(modes[m], ctx_frames[m]);
    if (wf <= 0) return open_refused("bad mode or ctx_frames");
    for (int j = 0; j < m; ++j)
      if (modes[j] == modes[m]) return open_refused("the models of a group must have pairwise distinct modes (vap, bc, nod)");
    if (m && follower_ports_out && follower_ports_out[m - 1] < 0) return open_refused("a follower's output port must be >= 0 (0 = ephemeral)");
    g->ports[m].mode = modes[m];
    g->ports[m].wf = wf;
    g->ports[m].off = acc;
    g->ports[m].R = frame_hzs[0] / frame_hzs[m];   // > 1: its echo history is sized with the staging (start)
    g->cfg_ports_out[m] = (m && follower_ports_out) ? follower_ports_out[m - 1] : 0;
    acc += (size_t)wf;
  }
  g->M = n_models;
  g->row_floats = acc;
  return VAPX_OK;
}

// The head and the tail every open call shares.  open_begin: the last open error is cleared and the caller's config, whatever its vintage,
// is read into *probe; false = a null argument (`args`) or a config of unknown size.  open_end: a front-end that did not come up is taken
// down again; a group's open always says why
bool open_begin(bool args, const vapx_ingest_config* cfg, vapx_ingest_config* probe) {
  g_open_error.clear();
  return args && read_config(cfg, probe);
}
int open_end(vapx_ingest* g, int rc, vapx_ingest_handle* out, bool group = false) {
  if (rc != VAPX_OK) {
    vapx_ingest_close(g);
    return group && g_open_error.empty() ? open_refused("could not allocate the staging blocks or bind the ports") : rc;
  }
  *out = g;
  return VAPX_OK;
}
}  // namespace

extern "C" {

int vapx_ingest_open_fn(vapx_ingest_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                        int32_t frame_hz, int32_t mode, const vapx_ingest_config* cfg, vapx_ingest_handle* out) {
  vapx_ingest_config probe;
  if (!open_begin(step && out, cfg, &probe)) return VAPX_E_INVAL;
  if (n_streams < 1 || max_batch < 1 || max_batch > n_streams) return VAPX_E_INVAL;
  if (!known_frame_hz(frame_hz)) return VAPX_E_INVAL;
  if (mode < 0 || mode > 2) return VAPX_E_INVAL;
  vapx_ingest* g = new vapx_ingest();
  g->step = step; g->reset = reset; g->user = user;
  g->S = n_streams; g->max_batch = max_batch; g->hz = frame_hz; g->ports[0].mode = mode;
  int rc = configure(g, cfg);
  if (rc == VAPX_OK) rc = start(g);
  return open_end(g, rc, out);
}

int vapx_ingest_open(vapx_handle engine, const vapx_ingest_config* cfg, vapx_ingest_handle* out) {
  vapx_ingest_config probe;
  if (!open_begin(engine && out, cfg, &probe)) return VAPX_E_INVAL;
  vapx_config ec;
  int rc = vapx_get_config(engine, &ec);
  if (rc != VAPX_OK) return rc;
  const EngineInput e = engine_input(engine);
  vapx_ingest* g = new vapx_ingest();
  g->engine = engine;
  g->step = engine_step; g->reset = engine_reset; g->user = g;
  g->S = ec.max_streams; g->max_batch = ec.max_batch; g->hz = ec.frame_hz; g->ports[0].mode = ec.mode;
  if (e.n_cls) g->set_class = engine_set_class;
  rc = configure(g, cfg, e);   // before the warm-up: a refused open leaves the engine untouched
  if (rc == VAPX_OK) {
    warm_up(g, vapx_step, VAPX_OUT_STRIDE, 3);
    rc = start(g);
  }
  return open_end(g, rc, out);
}

int32_t vapx_ingest_class_ports(vapx_ingest_handle g, int32_t* ports, int32_t max) {
  if (!g) return VAPX_E_INVAL;
  for (int c = 0; ports && c < g->tab_cls() && c < max; ++c) ports[c] = g->in_ports[c].port;
  return g->tab_cls();
}

int32_t vapx_ingest_stream_class(vapx_ingest_handle g, int32_t stream_id) {
  if (!g || !g->cls_table) return VAPX_E_INVAL;
  if (stream_id < 0 || stream_id >= g->S) return VAPX_E_RANGE;
  const int32_t* c = &g->tick_cls[(size_t)2 * stream_id];
  return c[0] == c[1] ? c[0] : VAPX_E_INVAL;   // a pair port's stream: vapx_ingest_stream_channel_classes
}

int32_t vapx_ingest_pair_ports(vapx_ingest_handle g, int32_t* ports, int32_t max) {
  if (!g) return VAPX_E_INVAL;
  const int n_pair = g->n_in - g->n_cls;      // the input ports behind the classes' own (none without a table)
  for (int p = 0; ports && p < n_pair && p < max; ++p) ports[p] = g->in_ports[g->n_cls + p].port;
  return n_pair;
}

int vapx_ingest_stream_channel_classes(vapx_ingest_handle g, int32_t stream_id, int32_t out[2]) {
  if (!g || !g->cls_table || !out) return VAPX_E_INVAL;
  if (stream_id < 0 || stream_id >= g->S) return VAPX_E_RANGE;
  out[0] = g->tick_cls[(size_t)2 * stream_id];
  out[1] = g->tick_cls[(size_t)2 * stream_id + 1];
  return VAPX_OK;
}

int vapx_ingest_ports(vapx_ingest_handle g, int32_t* port_in, int32_t* port_out) {
  if (!g) return VAPX_E_INVAL;
  if (port_in) *port_in = g->in_ports[0].port;
  if (port_out) *port_out = g->ports[0].port;
  return VAPX_OK;
}

int vapx_ingest_group_ports(vapx_ingest_handle g, int32_t* port_in, int32_t* ports_out, int32_t max_ports) {
  if (!g) return VAPX_E_INVAL;
  if (port_in) *port_in = g->in_ports[0].port;
  for (int m = 0; m < g->M && m < max_ports && ports_out; ++m) ports_out[m] = g->ports[m].port;
  return g->M;
}

const char* vapx_ingest_last_open_error(void) { return g_open_error.c_str(); }

int32_t vapx_wire_floats(int32_t mode, int32_t ctx_frames) {
  if (mode < VAPX_MODE_VAP || mode > VAPX_MODE_NOD || ctx_frames < 1 || ctx_frames > 512) return 0;
  return mode == VAPX_MODE_NOD ? ((VAPX_OUT_LOGITS + ctx_frames + 3) & ~3) : VAPX_OUT_LOGITS;
}

int vapx_ingest_open_group_fn(vapx_ingest_group_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                              int32_t frame_hz, int32_t ctx_frames, const int32_t* modes, int32_t n_models, const vapx_ingest_config* cfg,
                              const int32_t* follower_ports_out, vapx_ingest_handle* out) {
  const int32_t hzs[MAX_MODELS] = {frame_hz, frame_hz, frame_hz}, ctxs[MAX_MODELS] = {ctx_frames, ctx_frames, ctx_frames};
  if (n_models > MAX_MODELS) { g_open_error.clear(); return open_refused("a group serves one to three models"); }
  return vapx_ingest_open_group_fn2(step, reset, user, n_streams, max_batch, hzs, ctxs, modes, n_models, cfg, follower_ports_out, out);
}

int vapx_ingest_open_group_fn2(vapx_ingest_group_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                               const int32_t* frame_hzs, const int32_t* ctx_frames, const int32_t* modes, int32_t n_models,
                               const vapx_ingest_config* cfg, const int32_t* follower_ports_out, vapx_ingest_handle* out) {
  vapx_ingest_config probe;
  if (!open_begin(step && out && modes && frame_hzs && ctx_frames, cfg, &probe))
    return open_refused("null argument or a vapx_ingest_config of unknown size");
  if (n_streams < 1 || max_batch < 1 || max_batch > n_streams) return open_refused("need 1 <= max_batch <= n_streams");
  if (n_models < 1 || n_models > MAX_MODELS) return open_refused("a group serves one to three models");
  if (probe.n_input_classes)
    return open_refused("a trunk group's front-end takes no input classes: multi-port groups are not part of the class ports yet");
  if (!known_frame_hz(frame_hzs[0])) return open_refused("frame_hz must be 5, 10, 20 or 50");
  vapx_ingest* g = new vapx_ingest();
  g->step = step; g->reset = reset; g->user = user;
  g->S = n_streams; g->max_batch = max_batch; g->hz = frame_hzs[0];
  int rc = setup_group(g, frame_hzs, ctx_frames, modes, n_models, probe, follower_ports_out);
  if (rc == VAPX_OK) rc = configure(g, cfg);
  if (rc == VAPX_OK) rc = start(g);
  return open_end(g, rc, out, true);
}

int vapx_ingest_open_group(vapx_handle leader, const vapx_handle* followers, int32_t n_followers, const vapx_ingest_config* cfg,
                           const int32_t* follower_ports_out, vapx_ingest_handle* out) {
  vapx_ingest_config probe;
  if (!open_begin(leader && out && n_followers >= 0 && (!n_followers || followers), cfg, &probe))
    return open_refused("null argument or a vapx_ingest_config of unknown size");
  if (!vapx_step_group || !vapx_group_wire_floats) return open_refused("this build has no vapx_step_group");
  if (n_followers + 1 > MAX_MODELS) return open_refused("a group serves at most three models (vap, bc, nod)");
  vapx_config ec;
  int rc = vapx_get_config(leader, &ec);
  if (rc != VAPX_OK) return rc;
  int32_t modes[MAX_MODELS] = {ec.mode, 0, 0}, hzs[MAX_MODELS] = {ec.frame_hz, 0, 0}, ctxs[MAX_MODELS] = {ec.ctx_frames, 0, 0};
  for (int i = 0; i < n_followers; ++i) {   // each model's own rate and window (a mixed group: vapx.h, vapx_attach_trunk)
    vapx_config fc;
    if (!followers[i] || vapx_get_config(followers[i], &fc) != VAPX_OK) return open_refused("null follower");
    modes[i + 1] = fc.mode; hzs[i + 1] = fc.frame_hz; ctxs[i + 1] = fc.ctx_frames;
  }
  const EngineInput e = engine_input(leader);
  if (e.n_cls || probe.n_input_classes)
    return open_refused("a trunk group's front-end takes no input classes (the leader has a table, or the config names one): multi-port "
                        "groups are not part of the class ports yet; serve the leader alone, or the group without a table");
  vapx_ingest* g = new vapx_ingest();
  g->engine = leader;
  g->step = engine_group_step; g->reset = engine_reset; g->user = g;
  g->S = ec.max_streams; g->max_batch = ec.max_batch; g->hz = ec.frame_hz;
  rc = check_format(&probe, e.fmt);   // (ahead of the group's own refusals, as ever; configure finds nothing more in it)
  if (rc == VAPX_OK) rc = setup_group(g, hzs, ctxs, modes, n_followers + 1, probe, follower_ports_out);
  if (rc == VAPX_OK && g->row_floats != vapx_group_wire_floats(leader))
    rc = open_refused("`followers` are not the leader's attached followers (vapx_attach_trunk) in attach order");
  if (rc == VAPX_OK) rc = configure(g, cfg, e);
  if (rc == VAPX_OK) {
    int ticks = 3;   // every model's chain at least once: a slower follower's runs on every R-th tick
    for (int m = 0; m < g->M; ++m) ticks = std::max(ticks, g->ports[m].R);
    warm_up(g, vapx_step_group, g->row_floats, ticks);
    rc = start(g);
  }
  return open_end(g, rc, out, true);
}

int vapx_ingest_stats_read(vapx_ingest_handle g, vapx_ingest_stats* st, int32_t reset_latency_window) {
  if (!g || !st) return VAPX_E_INVAL;
  memset(st, 0, sizeof *st);
  st->frames_done = g->frames_done.load();
  st->ticks = g->ticks.load();
  st->rx_bytes = g->rx_bytes.load();
  st->tx_bytes = g->tx_bytes.load();
  st->in_connections = g->in_conns.load();
  st->out_connections = g->out_conns.load();
  st->dropped_listeners = g->dropped.load();
  st->numeric_resets = g->numeric_resets.load();
  st->overruns = g->overruns.load();
  st->mean_batch = st->ticks ? (double)g->batch_sum.load() / (double)st->ticks : 0.0;
  const int64_t c = g->lat.cnt.load();
  st->lat_mean_ms = c ? (double)g->lat.sum_us.load() / (double)c * 1e-3 : 0.0;
  st->lat_p50_ms = g->lat.pct(0.50);
  st->lat_p99_ms = g->lat.pct(0.99);
  st->lat_max_ms = (double)g->lat.max_us.load() * 1e-3;
  st->step_mean_ms = st->ticks ? (double)g->step_us.load() / (double)st->ticks * 1e-3 : 0.0;
  if (reset_latency_window) { g->lat.clear(); g->late10.store(0); }
  return VAPX_OK;
}

int vapx_ingest_late_read(vapx_ingest_handle g, int64_t* over_10ms, int64_t* answered) {
  if (!g) return VAPX_E_INVAL;
  if (over_10ms) *over_10ms = g->late10.load();
  if (answered) *answered = g->lat.cnt.load();
  return VAPX_OK;
}

void vapx_ingest_close(vapx_ingest_handle g) {
  if (!g) return;
  g->stop.store(true);
  g->ready_cv.notify_all();
  g->job_cv.notify_all();
  g->job_done_cv.notify_all();
  for (int fd : g->wake) kick(fd);
  if (g->accept_thread.joinable()) g->accept_thread.join();
  if (g->link_thread.joinable()) g->link_thread.join();
  if (g->link_fd >= 0) { std::lock_guard<std::mutex> lk(g->link_mu); g->link_fd = -1; }   // (the descriptor stays the caller's: include/vapx.h)
  if (g->ep_accept >= 0) close(g->ep_accept);
  for (auto& t : g->rx_threads) if (t.joinable()) t.join();
  if (g->tick_thread.joinable()) g->tick_thread.join();
  g->job_cv.notify_all();
  for (auto& t : g->tx_threads) if (t.joinable()) t.join();
  if (g->debug)
    fprintf(stderr, "[vapx ingest] longest rx pass %.2f ms, longest gap between busy rx passes %.2f ms, longest step %.2f ms, latency max %.2f ms, "
            "longest recv() %.2f ms, longest sendmsg() %.2f ms, longest tick fan-out (results ready -> last packet sent) %.2f ms\n",
            g->dbg_rx_pass_us.load() * 1e-3, g->dbg_rx_gap_us.load() * 1e-3, g->dbg_step_us.load() * 1e-3, (double)g->lat.max_us.load() * 1e-3,
            g->dbg_recv_us.load() * 1e-3, g->dbg_send_us.load() * 1e-3, g->dbg_job_tx_us.load() * 1e-3);
  if (g->debug && g->slots) {
    // streams whose results went nowhere (no output connection attached yet) or whose frames did not all come back out
    int shown = 0, odd = 0;
    for (int i = 0; i < g->S; ++i) {
      Slot& s = g->slots[i];
      const int64_t rdy = s.dbg_ready.load(), snt = s.dbg_sent.load(), nol = s.dbg_nolistener.load();
      if (nol == 0 && rdy == snt) continue;
      ++odd;
      if (shown++ < 24)
        fprintf(stderr, "[vapx ingest] slot %d: %ld frames assembled, %ld sent, %ld had NO listener; first frame ready %.3f s, listener attached %.3f s, first packet sent %.3f s (after the first slot's first frame)\n",
                i, (long)rdy, (long)snt, (long)nol, s.dbg_t_first_ready - g->slots[0].dbg_t_first_ready, s.dbg_t_attach - g->slots[0].dbg_t_first_ready,
                s.dbg_t_first_sent - g->slots[0].dbg_t_first_ready);
    }
    fprintf(stderr, "[vapx ingest] accept4 failures for lack of descriptors: %ld; CLOCK_MONOTONIC: inputs adopted %.3f .. %.3f, outputs adopted %.3f .. %.3f, slot 0's first frame %.3f\n",
            (long)g->accept_fd_errors.load(), g->dbg_t_in_first, g->dbg_t_in_last, g->dbg_t_out_first, g->dbg_t_out_last, g->slots[0].dbg_t_first_ready);
    fprintf(stderr, "[vapx ingest] %d of %d slots lost results to a missing listener or did not send every assembled frame\n", odd, g->S);
  }
  if (g->slots) {
    for (int i = 0; i < g->S; ++i) {
      if (g->slots[i].fd_in >= 0) close(g->slots[i].fd_in);
      for (auto& l : g->slots[i].listeners) for (int fd : l) close(fd);
    }
  }
  for (auto& o : g->ports) { for (int fd : o.out_all) close(fd); if (o.lsock >= 0) close(o.lsock); }
  for (const InPort& ip : g->in_ports) if (ip.lsock >= 0) close(ip.lsock);
  for (int fd : g->ep) close(fd);
  for (int fd : g->wake) close(fd);
  auto drop = [&](void* p) {
    if (!p) return;
    if (g->pinned_blocks) vapx_host_free(p); else free(p);
  };
  drop(g->stage);
  drop(g->batch_audio);
  drop(g->jobs[0].out);
  drop(g->jobs[1].out);
  delete g;
}

// ---- one front door for N per-GPU front-ends ------------------------------------------------------------------------------------
// The reference listens on ONE port pair (vap_main.py:338-366).  N GPUs = N passive shards (each with its own engine, receive / tick /
// send threads) behind one accept thread on that pair.  Dialogue slots are numbered GLOBALLY g = local_slot * N + shard, so that
//   - a new input connection takes the lowest free global slot: GPUs fill evenly at any load (round-robin), and a dialogue that
//     reconnects while its slot is still the lowest free one lands on the GPU that holds its state (ring, LSTM) — stickiness;
//   - the k-th output connection hears the k-th dialogue, exactly as a single front-end does (fewest listeners, lowest global slot).
// A dialogue never moves between GPUs: its state lives there (vapx_get_state / vapx_set_state migrate one on purpose).
}  // extern "C"

struct RemoteShard {                        // the door's mirror of a shard that lives in another process
  int link = -1, S = 0, hz = 0, mode = 0;
  bool broadcast = false, dead = false;
  std::vector<char> used;                   // input slot taken
  int free_hint = 0;
  std::vector<int> lcount;                  // listeners per slot
  int lmin = 0, lcursor = 0, bcast = 0;
  int lowest_free() {
    for (int i = free_hint; i < S; ++i) if (!used[i]) { free_hint = i; return i; }
    free_hint = S;
    return -1;
  }
  std::pair<int, int> next_listener() {
    if (broadcast) return {bcast, 0};
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = lcursor; i < S; ++i) if (lcount[i] == lmin) { lcursor = i; return {lmin, i}; }
      ++lmin; lcursor = 0;
    }
    return {lmin, 0};
  }
};

struct vapx_frontdoor {
  std::vector<vapx_ingest*> shards;
  std::vector<RemoteShard> remote;          // vapx_frontdoor_open_links: shards in other processes
  int lin = -1, lout = -1, port_in = 0, port_out = 0, ep = -1;
  std::thread th;
  std::atomic<bool> stop{false};
  std::atomic<int64_t> accepted_in{0}, accepted_out{0}, refused{0};
};

namespace {

void frontdoor_main(vapx_frontdoor* d) {
  epoll_event evs[8];
  const int N = (int)d->shards.size();
  while (!d->stop.load()) {
    int n = epoll_wait(d->ep, evs, 8, 100);
    for (int i = 0; i < n; ++i) {
      const uint64_t kind = evs[i].data.u64 & ~0xffffffffull;
      for (;;) {
        int fd = accept4(kind == K_LISTEN_IN ? d->lin : d->lout, nullptr, nullptr, SOCK_NONBLOCK);
        if (fd < 0) {
          // out of descriptors: the listen socket stays readable (level-triggered), so epoll_wait would return at once and this thread
          // would spin at 100 % — back off until a connection closes
          if (errno == EMFILE || errno == ENFILE || errno == ENOBUFS || errno == ENOMEM) std::this_thread::sleep_for(std::chrono::milliseconds(20));
          break;
        }
        if (kind == K_LISTEN_IN) {
          bool placed = false;
          for (int attempt = 0; attempt < N && !placed; ++attempt) {      // (a shard can fill up between the query and the adoption)
            long best = -1; int who = -1;
            for (int k = 0; k < N; ++k) {
              const int ls = lowest_free_slot(d->shards[k]);
              if (ls < 0) continue;
              const long gslot = (long)ls * N + k;
              if (who < 0 || gslot < best) { best = gslot; who = k; }
            }
            if (who < 0) break;
            placed = adopt_in(d->shards[who], fd);
          }
          if (placed) d->accepted_in.fetch_add(1);
          else { close(fd); d->refused.fetch_add(1); }               // every dialogue slot of every GPU is taken
        } else {
          int who = 0; long bestc = -1, bestg = -1;
          for (int k = 0; k < N; ++k) {
            // a broadcast shard (one dialogue slot: serve.py's default --streams 1) is ONE candidate: (its listener count, slot 0) — so the
            // k-th output connection hears GPU k mod N's dialogue instead of every listener piling up on shard 0
            std::pair<int, int> c;
            if (d->shards[k]->broadcast) { std::lock_guard<std::mutex> lk(d->shards[k]->slots_mu); c = {(int)d->shards[k]->ports[0].out_all.size(), 0}; }
            else c = next_listener_slot(d->shards[k]);
            const long gslot = (long)c.second * N + k;
            if (bestc < 0 || c.first < bestc || (c.first == bestc && gslot < bestg)) { bestc = c.first; bestg = gslot; who = k; }
          }
          adopt_out(d->shards[who], fd);
          d->accepted_out.fetch_add(1);
        }
      }
    }
  }
}

constexpr uint64_t K_LINK = 4ull << 32;

// The same door with the shards in OTHER processes (one per GPU): placement runs on the mirrors, the accepted socket travels to the worker
// (SCM_RIGHTS) and is closed here - this process never holds more than the listen sockets, the links and the connection in hand.
void frontdoor_remote_main(vapx_frontdoor* d) {
  epoll_event evs[16];
  const int N = (int)d->remote.size();
  while (!d->stop.load()) {
    int n = epoll_wait(d->ep, evs, 16, 100);
    for (int i = 0; i < n; ++i) {
      const uint64_t kind = evs[i].data.u64 & ~0xffffffffull;
      if (kind == K_LINK) {                  // a worker reports a released slot / a dropped listener (or went away)
        RemoteShard& r = d->remote[(int)(evs[i].data.u64 & 0xffffffffu)];
        for (;;) {
          LinkMsg m;
          const int rc = link_recv(r.link, &m, nullptr, 0);
          if (rc == 0) break;
          if (rc < 0) { if (!r.dead) { r.dead = true; epoll_ctl(d->ep, EPOLL_CTL_DEL, r.link, nullptr); } break; }
          if (m.kind == LK_IN_CLOSED && m.a >= 0 && m.a < r.S) { r.used[m.a] = 0; if (m.a < r.free_hint) r.free_hint = m.a; }
          else if (m.kind == LK_OUT_CLOSED) {
            if (r.broadcast || m.a < 0) { if (r.bcast > 0) --r.bcast; }
            else if (m.a < r.S && r.lcount[m.a] > 0) {
              if (--r.lcount[m.a] < r.lmin) { r.lmin = r.lcount[m.a]; r.lcursor = m.a; }
              else if (r.lcount[m.a] == r.lmin && m.a < r.lcursor) r.lcursor = m.a;
            }
          }
        }
        continue;
      }
      for (;;) {
        int fd = accept4(kind == K_LISTEN_IN ? d->lin : d->lout, nullptr, nullptr, SOCK_NONBLOCK);
        if (fd < 0) {
          if (errno == EMFILE || errno == ENFILE || errno == ENOBUFS || errno == ENOMEM) std::this_thread::sleep_for(std::chrono::milliseconds(20));
          break;
        }
        if (kind == K_LISTEN_IN) {
          long best = -1; int who = -1, ls_who = -1;
          for (int k = 0; k < N; ++k) {
            if (d->remote[k].dead) continue;
            const int ls = d->remote[k].lowest_free();
            if (ls < 0) continue;
            const long gslot = (long)ls * N + k;
            if (who < 0 || gslot < best) { best = gslot; who = k; ls_who = ls; }
          }
          if (who >= 0 && link_send(d->remote[who].link, nullptr, LinkMsg{LK_ADOPT_IN, ls_who, 0, 0}, fd)) {
            d->remote[who].used[ls_who] = 1;
            d->accepted_in.fetch_add(1);
          } else d->refused.fetch_add(1);      // every dialogue slot of every GPU is taken (or that worker is gone)
        } else {
          int who = -1, slot = 0; long bestc = -1, bestg = -1;
          for (int k = 0; k < N; ++k) {
            if (d->remote[k].dead) continue;
            const std::pair<int, int> c = d->remote[k].next_listener();
            const long gslot = (long)c.second * N + k;
            if (bestc < 0 || c.first < bestc || (c.first == bestc && gslot < bestg)) { bestc = c.first; bestg = gslot; who = k; slot = c.second; }
          }
          if (who >= 0 && link_send(d->remote[who].link, nullptr, LinkMsg{LK_ADOPT_OUT, slot, 0, 0}, fd)) {
            RemoteShard& r = d->remote[who];
            if (r.broadcast) ++r.bcast; else { ++r.lcount[slot]; r.lcursor = slot + 1; }
            d->accepted_out.fetch_add(1);
          } else d->refused.fetch_add(1);
        }
        close(fd);                           // the worker holds its own copy now
      }
    }
  }
}

}  // namespace

extern "C" {

int vapx_ingest_attach_link(vapx_ingest_handle g, int32_t link_fd) {
  if (!g || link_fd < 0 || g->link_fd >= 0) return VAPX_E_INVAL;
  if (g->in_ports[0].lsock >= 0 || g->ports[0].lsock >= 0) return VAPX_E_INVAL;   // only a passive shard takes its connections from a door
  g->link_fd = link_fd;
  if (!link_send(link_fd, &g->link_mu, LinkMsg{LK_HELLO, g->S, g->hz, g->ports[0].mode | (g->broadcast ? 256 : 0)})) { g->link_fd = -1; return VAPX_E_INVAL; }
  g->link_thread = std::thread(link_main, g);
  return VAPX_OK;
}

int vapx_frontdoor_open_links(const int32_t* link_fds, int32_t n_links, int32_t port_in, int32_t port_out, int32_t bind_any, vapx_frontdoor_handle* out) {
  if (!link_fds || n_links < 1 || !out || port_in < 0 || port_out < 0) return VAPX_E_INVAL;
  vapx_frontdoor* d = new vapx_frontdoor();
  d->remote.resize(n_links);
  for (int k = 0; k < n_links; ++k) {        // every worker introduces itself (it may still be loading its weights: wait up to 5 minutes)
    RemoteShard& r = d->remote[k];
    r.link = link_fds[k];
    LinkMsg m;
    int rc = 0;
    for (int waited = 0; waited < 3000 && rc == 0; ++waited) rc = link_recv(r.link, &m, nullptr, 100);
    if (rc <= 0 || m.kind != LK_HELLO || m.a < 1) { delete d; return VAPX_E_INVAL; }
    r.S = m.a; r.hz = m.b; r.mode = m.c & 255; r.broadcast = (m.c & 256) != 0;
    r.used.assign(r.S, 0); r.lcount.assign(r.S, 0);
    if (r.hz != d->remote[0].hz || r.mode != d->remote[0].mode) { delete d; return VAPX_E_INVAL; }
  }
  d->lin = listen_on(port_in, bind_any != 0, &d->port_in);
  d->lout = listen_on(port_out, bind_any != 0, &d->port_out);
  if (d->lin < 0 || d->lout < 0) { vapx_frontdoor_close(d); return VAPX_E_INVAL; }
  d->ep = epoll_create1(0);
  ep_add(d->ep, d->lin, K_LISTEN_IN);
  ep_add(d->ep, d->lout, K_LISTEN_OUT);
  for (int k = 0; k < n_links; ++k) ep_add(d->ep, d->remote[k].link, K_LINK | (uint32_t)k);
  d->th = std::thread(frontdoor_remote_main, d);
  *out = d;
  return VAPX_OK;
}

int vapx_frontdoor_open(vapx_ingest_handle* shards, int32_t n_shards, int32_t port_in, int32_t port_out, int32_t bind_any,
                        vapx_frontdoor_handle* out) {
  if (!shards || n_shards < 1 || !out || port_in < 0 || port_out < 0) return VAPX_E_INVAL;
  for (int k = 0; k < n_shards; ++k) {
    if (!shards[k] || shards[k]->in_ports[0].lsock >= 0 || shards[k]->ports[0].lsock >= 0 || shards[k]->M != 1) return VAPX_E_INVAL;   // shards must be passive (port_in = port_out = -1)
    if (shards[k]->hz != shards[0]->hz || shards[k]->ports[0].mode != shards[0]->ports[0].mode) return VAPX_E_INVAL;
  }
  vapx_frontdoor* d = new vapx_frontdoor();
  d->shards.assign(shards, shards + n_shards);
  d->lin = listen_on(port_in, bind_any != 0, &d->port_in);
  d->lout = listen_on(port_out, bind_any != 0, &d->port_out);
  if (d->lin < 0 || d->lout < 0) { vapx_frontdoor_close(d); return VAPX_E_INVAL; }
  d->ep = epoll_create1(0);
  ep_add(d->ep, d->lin, K_LISTEN_IN);
  ep_add(d->ep, d->lout, K_LISTEN_OUT);
  d->th = std::thread(frontdoor_main, d);
  *out = d;
  return VAPX_OK;
}

int vapx_frontdoor_ports(vapx_frontdoor_handle d, int32_t* port_in, int32_t* port_out) {
  if (!d) return VAPX_E_INVAL;
  if (port_in) *port_in = d->port_in;
  if (port_out) *port_out = d->port_out;
  return VAPX_OK;
}

int vapx_frontdoor_counts(vapx_frontdoor_handle d, int64_t* accepted_in, int64_t* accepted_out, int64_t* refused) {
  if (!d) return VAPX_E_INVAL;
  if (accepted_in) *accepted_in = d->accepted_in.load();
  if (accepted_out) *accepted_out = d->accepted_out.load();
  if (refused) *refused = d->refused.load();
  return VAPX_OK;
}

void vapx_frontdoor_close(vapx_frontdoor_handle d) {
  if (!d) return;
  d->stop.store(true);
  if (d->th.joinable()) d->th.join();
  if (d->ep >= 0) close(d->ep);
  if (d->lin >= 0) close(d->lin);
  if (d->lout >= 0) close(d->lout);
  delete d;                                  // the shards stay open: close them with vapx_ingest_close
}

int64_t vapx_wire_decode_input(const uint8_t* bytes, size_t n_bytes, double gain, float* x1_f32, float* x2_f32, double* x1_f64,
                               double* x2_f64) {
  if (!bytes || n_bytes % PAIR_BYTES) return VAPX_E_INVAL;   // util.conv_bytearray_2_2floatarray needs whole f64 pairs
  const size_t n = n_bytes / PAIR_BYTES;
  constexpr size_t CH = 256;   // pairs per pass: an output the caller left out is written to a scratch on the stack, and dropped
  double no_d[CH];
  float no_f[CH];
  for (size_t i = 0; i < n; i += CH) {
    double* d[2] = {x1_f64 ? x1_f64 + i : no_d, x2_f64 ? x2_f64 + i : no_d};
    float* f[2] = {x1_f32 ? x1_f32 + i : no_f, x2_f32 ? x2_f32 + i : no_f};
    move_f64<2>(bytes + i * PAIR_BYTES, std::min(CH, n - i), gain, d, f);
  }
  return (int64_t)n;
}

int64_t vapx_wire_encode_result(int32_t mode, double t, const double* x1, const double* x2, int32_t n, const float* row, uint8_t* dst,
                                size_t cap) {
  if (mode < 0 || mode > 2 || !x1 || !x2 || n < 0 || !row) return VAPX_E_INVAL;
  const int nr = mode == VAPX_MODE_NOD ? (int)row[VAPX_OUT_NVALID] : 0;
  if (nr < 0 || nr > 256) return VAPX_E_INVAL;
  const size_t plen = 8 + 2 * (4 + 8 * (size_t)n) + (size_t)tail_bytes(mode, nr);
  if (!dst || cap < 4 + plen) return (int64_t)(4 + plen);
  uint8_t* p = dst;
  put_u32(p, (uint32_t)plen);
  put_f64(p, t);
  put_u32(p, (uint32_t)n);
  memcpy(p, x1, (size_t)n * 8); p += (size_t)n * 8;
  put_u32(p, (uint32_t)n);
  memcpy(p, x2, (size_t)n * 8); p += (size_t)n * 8;
  p += encode_tail(mode, row, p);
  return (int64_t)(p - dst);
}

}  // extern "C"
