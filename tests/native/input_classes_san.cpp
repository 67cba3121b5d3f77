// Sanitizer harness for the class ports of the native TCP front-end (vap-realtime_amd/csrc/ingest.cpp, vapx.h "Input classes"): the
// front-end is compiled INTO this program next to stubs of the engine entry points it links against, opened over a step FUNCTION with a
// class table, and driven by in-process clients: dialogues on three class ports at once, the step function walking the packed block by
// vapx_ingest_stream_class, reconnects on ANOTHER class's port in the middle of a frame, and a close under load.  Built with
// -fsanitize=address,undefined (and with -fsanitize=thread) and run on its own by tests/test_input_classes.py; any report fails the test.
#include "../../vap-realtime_amd/csrc/ingest.cpp"

#include <atomic>
#include <cstdlib>

extern "C" {
void* vapx_host_alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
void vapx_host_free(void* p) { free(p); }
int vapx_get_config(vapx_handle, vapx_config*) { return VAPX_E_INVAL; }
int vapx_reset_stream(vapx_handle, int32_t) { return VAPX_E_INVAL; }
int vapx_reset_carry(vapx_handle, int32_t) { return VAPX_E_INVAL; }
int vapx_step(vapx_handle, int32_t, const int32_t*, const float*, int32_t, float*, int32_t, void*) { return VAPX_E_INVAL; }
int32_t vapx_bad_slots(vapx_handle, int32_t*, int32_t) { return 0; }
const char* vapx_last_error(vapx_handle) { return "stub"; }
}

namespace {

constexpr int HZ = 50, NCLS = 3;
const vapx_input_class kTable[NCLS] = {{16000, VAPX_PCM_F32}, {8000, VAPX_PCM_MULAW}, {48000, VAPX_PCM_S16}};
const int kHop[NCLS] = {16000 / HZ, 8000 / HZ, 48000 / HZ};
const int kBps[NCLS] = {4, 1, 2};          // bytes per sample of the staging
const int kPair[NCLS] = {16, 2, 4};        // bytes of a (ch1, ch2) pair on the wire
vapx_ingest_handle g_front = nullptr;
std::atomic<long> g_steps{0}, g_bad_blocks{0};

// every sample a client of class c sends is the byte pattern of `tag` (f64: the value itself), so a slot read at a wrong offset shows
uint8_t tag_byte(int c, int tag) { return (uint8_t)(0x10 * (c + 1) + tag); }

int step_fn(void*, int32_t n, const int32_t* ids, const float* audio, float* out) {
  const uint8_t* p = (const uint8_t*)audio;
  for (int i = 0; i < n; ++i) {
    const int c = vapx_ingest_stream_class(g_front, ids[i]);
    float* o = out + (size_t)i * VAPX_OUT_STRIDE;
    memset(o, 0, VAPX_OUT_STRIDE * sizeof(float));
    if (c < 0 || c >= NCLS) { g_bad_blocks.fetch_add(1); return VAPX_E_INVAL; }
    const size_t nb = (size_t)2 * kHop[c] * kBps[c];
    // the slot's first and last sample must be of class c: f32 1.0 + c, or the class's byte pattern
    if (c == 0) {
      float a, z;
      memcpy(&a, p, 4); memcpy(&z, p + nb - 4, 4);
      if (a != 1.0f || z != -1.0f) g_bad_blocks.fetch_add(1);
    } else if ((p[0] >> 4) != c + 1 || (p[nb - 1] >> 4) != c + 1) g_bad_blocks.fetch_add(1);
    o[0] = (float)c; o[1] = (float)ids[i];
    o[VAPX_OUT_NVALID] = 1.f;
    p += nb;
  }
  g_steps.fetch_add(1);
  return 0;
}
void reset_fn(void*, int32_t) {}

int dial(int port) {
  int s = socket(AF_INET, SOCK_STREAM, 0);
  sockaddr_in a;
  memset(&a, 0, sizeof a);
  a.sin_family = AF_INET;
  a.sin_port = htons((uint16_t)port);
  inet_pton(AF_INET, "127.0.0.1", &a.sin_addr);
  for (int t = 0; t < 200; ++t) {
    if (connect(s, (sockaddr*)&a, sizeof a) == 0) return s;
    usleep(5000);
  }
  perror("connect");
  exit(3);
}

bool send_all(int fd, const void* p, size_t n) {
  const char* c = (const char*)p;
  while (n) {
    ssize_t w = send(fd, c, n, MSG_NOSIGNAL);
    if (w <= 0) { if (errno == EINTR) continue; return false; }
    c += w; n -= (size_t)w;
  }
  return true;
}

// `frames` frames of class c in 10 ms packets (input_hz / 100 pairs each); stop_after_packets >= 0: vanish in the middle of a frame
void send_frames(int fd, int c, int tag, int frames, int stop_after_packets = -1) {
  const int pairs = kTable[c].input_hz / 100;
  std::vector<uint8_t> pk((size_t)pairs * kPair[c]);
  if (c == 0) {
    for (int i = 0; i < pairs; ++i) { const double a = 1.0, b = -1.0; memcpy(&pk[16 * i], &a, 8); memcpy(&pk[16 * i + 8], &b, 8); }
  } else memset(pk.data(), tag_byte(c, tag), pk.size());
  int sent = 0;
  for (int f = 0; f < frames; ++f)
    for (int p = 0; p < 100 / HZ; ++p) {
      if (stop_after_packets >= 0 && sent == stop_after_packets) return;
      if (!send_all(fd, pk.data(), pk.size())) return;
      ++sent;
    }
}

// result packets until `want` arrived or the peer closed / timed out: the echo must have the class's hop_in samples, p_now[0] its class
int read_results(int fd, int want, int c, std::atomic<long>* wrong) {
  timeval tv{5, 0};
  setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  int got = 0;
  while (got < want) {
    ssize_t r = recv(fd, tmp, sizeof tmp, 0);
    if (r <= 0) break;
    buf.insert(buf.end(), tmp, tmp + r);
    size_t off = 0;
    while (buf.size() - off >= 4) {
      uint32_t len;
      memcpy(&len, buf.data() + off, 4);
      if (buf.size() - off < 4 + (size_t)len) break;
      const uint8_t* b = buf.data() + off + 4;   // f64 t, u32 n, x1[n], u32 n, x2[n], u32 2, p_now[2], ...
      uint32_t n1;
      memcpy(&n1, b + 8, 4);
      double pnow0 = -1;
      if (n1 == (uint32_t)kHop[c]) memcpy(&pnow0, b + 8 + 2 * (4 + 8 * (size_t)n1) + 4, 8);
      if (n1 != (uint32_t)kHop[c] || pnow0 != (double)c) wrong->fetch_add(1);
      off += 4 + len;
      ++got;
    }
    if (off) buf.erase(buf.begin(), buf.begin() + off);
  }
  return got;
}

}  // namespace

int main() {
  const int PER = 4, S = NCLS * PER, FRAMES = 30;
  vapx_ingest_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  cfg.rx_threads = 3; cfg.tx_threads = 2; cfg.max_wait_us = 300; cfg.reset_on_connect = 1; cfg.gain = 1;
  cfg.n_input_classes = NCLS;
  for (int c = 0; c < NCLS; ++c) cfg.input_classes[c] = kTable[c];
  if (vapx_ingest_open_fn(step_fn, reset_fn, nullptr, S, S, HZ, VAPX_MODE_VAP, &cfg, &g_front) != 0) {
    fprintf(stderr, "open failed: %s\n", vapx_ingest_last_open_error());
    return 2;
  }
  int ports[NCLS] = {0, 0, 0}, pin = 0, pout = 0;
  if (vapx_ingest_class_ports(g_front, ports, NCLS) != NCLS) return 2;
  vapx_ingest_ports(g_front, &pin, &pout);
  std::atomic<long> wrong{0}, answered{0};
  // ---- phase 1: PER dialogues per class, connected class by class (slots c * PER ..), every frame answered in its own class ----
  std::vector<int> fin(S), fout(S);
  for (int i = 0; i < S; ++i) { fin[i] = dial(ports[i / PER]); usleep(20000); }   // one after another: dialogue i takes slot i
  for (int i = 0; i < S; ++i) { fout[i] = dial(pout); usleep(5000); }             // the k-th output connection listens to the k-th stream
  usleep(100000);
  {
    std::vector<std::thread> th;
    for (int i = 0; i < S; ++i) {
      th.emplace_back([&, i] { send_frames(fin[i], i / PER, i % PER, FRAMES); });
      th.emplace_back([&, i] { answered.fetch_add(read_results(fout[i], FRAMES, i / PER, &wrong)); });
    }
    for (auto& t : th) t.join();
  }
  if (answered.load() != (long)S * FRAMES || wrong.load() || g_bad_blocks.load()) {
    fprintf(stderr, "phase 1: answered %ld of %d, %ld in a wrong class, %ld packed blocks with a slot at a wrong offset\n", answered.load(), S * FRAMES,
            wrong.load(), g_bad_blocks.load());
    return 4;
  }
  // ---- phase 2: churn across classes - every other dialogue dies in the middle of a frame and comes back on the NEXT class's port ----
  std::vector<int> cls(S);
  for (int i = 0; i < S; ++i) cls[i] = i / PER;
  for (int round = 0; round < 3; ++round) {
    for (int i = round % 2; i < S; i += 2) {   // one at a time: the freed slot is the only free one, the dialogue returns to it
      send_frames(fin[i], cls[i], i % PER, 1, 1);   // half a frame, then gone: nothing of it is ever answered
      close(fin[i]);
      usleep(20000);
      cls[i] = (cls[i] + 1) % NCLS;
      fin[i] = dial(ports[cls[i]]);
      usleep(20000);
    }
    std::vector<std::thread> t2;
    answered.store(0);
    for (int i = 0; i < S; ++i) {
      t2.emplace_back([&, i] { send_frames(fin[i], cls[i], i % PER, 5); });
      t2.emplace_back([&, i] { answered.fetch_add(read_results(fout[i], 5, cls[i], &wrong)); });
    }
    for (auto& t : t2) t.join();
    if (answered.load() != (long)S * 5 || wrong.load() || g_bad_blocks.load()) {
      fprintf(stderr, "phase 2 round %d: answered %ld of %d, %ld in a wrong class, %ld bad blocks\n", round, answered.load(), S * 5, wrong.load(),
              g_bad_blocks.load());
      return 5;
    }
  }
  // ---- phase 3: close while a third of the senders are still pushing ----
  std::atomic<bool> stop{false};
  std::vector<std::thread> t4;
  for (int i = 0; i < S; i += 3) t4.emplace_back([&, i] { while (!stop.load()) send_frames(fin[i], cls[i], i % PER, 2); });
  usleep(100000);
  vapx_ingest_stats st;
  vapx_ingest_stats_read(g_front, &st, 1);
  vapx_ingest_close(g_front);
  stop.store(true);
  for (auto& t : t4) t.join();
  for (int fd : fin) close(fd);
  for (int fd : fout) close(fd);
  printf("ok: %d dialogues on %d class ports, steps %ld, frames_done %ld, bad blocks %ld\n", S, NCLS, g_steps.load(), (long)st.frames_done, g_bad_blocks.load());
  return g_bad_blocks.load() ? 6 : 0;
}
