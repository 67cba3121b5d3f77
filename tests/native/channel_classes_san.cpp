// Sanitizer harness for the PAIR ports of the native TCP front-end (vap-realtime_amd/csrc/ingest.cpp, vapx.h "Input classes", CHANNEL
// CLASSES): the front-end is compiled INTO this program next to stubs of the engine entry points it links against, opened over a step
// FUNCTION with a class table and three pair ports, and driven by in-process clients that send PLANAR packets in odd-sized pieces (so that
// packets, channels and f64 samples are split across reads), next to one plain class port.  The step function walks the packed block by
// vapx_ingest_stream_channel_classes and checks both rows of every slot.  Then dialogues die in the middle of a frame and come back on
// ANOTHER pair port, and the front-end is closed under load.  Built with -fsanitize=address,undefined and run on its own by
// tests/test_channel_classes.py; any report fails the test.
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

constexpr int HZ = 50, NCLS = 3, NPORT = 4;   // ports 0 .. 2: pair ports, port 3: the class port of class 2
const vapx_input_class kTable[NCLS] = {{16000, VAPX_PCM_F32}, {8000, VAPX_PCM_MULAW}, {48000, VAPX_PCM_S16}};
const int kHop[NCLS] = {16000 / HZ, 8000 / HZ, 48000 / HZ};
const int kBps[NCLS] = {4, 1, 2};             // bytes per sample of the staging
const int kWire[NCLS] = {8, 1, 2};            // bytes per sample on the wire
const int kOf[NPORT][2] = {{1, 2}, {0, 1}, {2, 2}, {2, 2}};   // the channel classes of a connection on port p
vapx_ingest_handle g_front = nullptr;
std::atomic<long> g_steps{0}, g_bad_blocks{0};

// channel ch of a raw class sends the byte 0x10 * (c + 1) + ch all over, an f64 class the value 1.0 + ch
bool row_ok(int c, int ch, const uint8_t* p) {
  const size_t nb = (size_t)kHop[c] * kBps[c];
  if (c == 0) {
    float a, z;
    memcpy(&a, p, 4); memcpy(&z, p + nb - 4, 4);
    return a == 1.0f + ch && z == 1.0f + ch;
  }
  const uint8_t want = (uint8_t)(0x10 * (c + 1) + ch);
  return p[0] == want && p[nb / 2] == want && p[nb - 1] == want;
}

int step_fn(void*, int32_t n, const int32_t* ids, const float* audio, float* out) {
  const uint8_t* p = (const uint8_t*)audio;
  for (int i = 0; i < n; ++i) {
    int32_t c[2] = {-1, -1};
    float* o = out + (size_t)i * VAPX_OUT_STRIDE;
    memset(o, 0, VAPX_OUT_STRIDE * sizeof(float));
    if (vapx_ingest_stream_channel_classes(g_front, ids[i], c) != 0 || c[0] < 0 || c[0] >= NCLS || c[1] < 0 || c[1] >= NCLS) {
      g_bad_blocks.fetch_add(1);
      return VAPX_E_INVAL;
    }
    for (int ch = 0; ch < 2; ++ch) {   // channel 1's row, then channel 2's
      if (!row_ok(c[ch], ch, p)) g_bad_blocks.fetch_add(1);
      p += (size_t)kHop[c[ch]] * kBps[c[ch]];
    }
    o[0] = (float)(10 * c[0] + c[1]); o[1] = (float)ids[i];
    o[VAPX_OUT_NVALID] = 1.f;
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

// one 10 ms packet of port p: planar on a pair port (channel 1's samples, then channel 2's), interleaved pairs on the class port
std::vector<uint8_t> packet(int p) {
  std::vector<uint8_t> pk;
  if (p == 3) {
    pk.resize((size_t)kTable[2].input_hz / 100 * 4);
    for (size_t i = 0; i < pk.size(); i += 4) { pk[i] = pk[i + 1] = 0x30; pk[i + 2] = pk[i + 3] = 0x31; }
    return pk;
  }
  for (int ch = 0; ch < 2; ++ch) {
    const int c = kOf[p][ch], ns = kTable[c].input_hz / 100;
    const size_t at = pk.size();
    pk.resize(at + (size_t)ns * kWire[c]);
    if (c == 0) {
      const double v = 1.0 + ch;
      for (int i = 0; i < ns; ++i) memcpy(&pk[at + 8 * (size_t)i], &v, 8);
    } else memset(&pk[at], 0x10 * (c + 1) + ch, (size_t)ns * kWire[c]);
  }
  return pk;
}

// `frames` frames of port p's packets, sent in pieces of `piece` bytes; stop_after_bytes >= 0: vanish in the middle of a frame
void send_frames(int fd, int p, int frames, size_t piece, long stop_after_bytes = -1) {
  const std::vector<uint8_t> pk = packet(p);
  std::vector<uint8_t> all;
  for (int i = 0; i < frames * (100 / HZ); ++i) all.insert(all.end(), pk.begin(), pk.end());
  if (stop_after_bytes >= 0) all.resize(std::min(all.size(), (size_t)stop_after_bytes));
  for (size_t at = 0; at < all.size(); at += piece)
    if (!send_all(fd, all.data() + at, std::min(piece, all.size() - at))) return;
}

// result packets until `want` arrived or the peer closed / timed out: x1 and x2 must have their own classes' hop_in samples
int read_results(int fd, int want, int p, std::atomic<long>* wrong) {
  timeval tv{5, 0};
  setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  int got = 0;
  const uint32_t h1 = (uint32_t)kHop[kOf[p][0]], h2 = (uint32_t)kHop[kOf[p][1]];
  while (got < want) {
    ssize_t r = recv(fd, tmp, sizeof tmp, 0);
    if (r <= 0) break;
    buf.insert(buf.end(), tmp, tmp + r);
    size_t off = 0;
    while (buf.size() - off >= 4) {
      uint32_t len;
      memcpy(&len, buf.data() + off, 4);
      if (buf.size() - off < 4 + (size_t)len) break;
      const uint8_t* b = buf.data() + off + 4;   // f64 t, u32 n1, x1[n1], u32 n2, x2[n2], u32 2, p_now[2], ...
      uint32_t n1, n2 = 0;
      memcpy(&n1, b + 8, 4);
      double pnow0 = -1, first2 = 0;
      if (n1 == h1) memcpy(&n2, b + 12 + 8 * (size_t)n1, 4);
      if (n1 == h1 && n2 == h2) {
        memcpy(&first2, b + 16 + 8 * (size_t)n1, 8);
        memcpy(&pnow0, b + 16 + 8 * ((size_t)n1 + n2) + 4, 8);
      }
      if (n1 != h1 || n2 != h2 || pnow0 != (double)(10 * kOf[p][0] + kOf[p][1]) || first2 == 0) wrong->fetch_add(1);
      off += 4 + len;
      ++got;
    }
    if (off) buf.erase(buf.begin(), buf.begin() + off);
  }
  return got;
}

}  // namespace

int main() {
  const int PER = 3, S = NPORT * PER, FRAMES = 30;
  const size_t kPiece[4] = {333, 1 << 20, 7, 1001};
  vapx_ingest_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  cfg.rx_threads = 3; cfg.tx_threads = 2; cfg.max_wait_us = 300; cfg.reset_on_connect = 1; cfg.gain = 1;
  cfg.n_input_classes = NCLS;
  for (int c = 0; c < NCLS; ++c) cfg.input_classes[c] = kTable[c];
  cfg.n_pair_ports = 3;
  for (int p = 0; p < 3; ++p) { cfg.pair_ports[p].cls_ch1 = kOf[p][0]; cfg.pair_ports[p].cls_ch2 = kOf[p][1]; }
  if (vapx_ingest_open_fn(step_fn, reset_fn, nullptr, S, S, HZ, VAPX_MODE_VAP, &cfg, &g_front) != 0) {
    fprintf(stderr, "open failed: %s\n", vapx_ingest_last_open_error());
    return 2;
  }
  int ports[NPORT] = {0, 0, 0, 0}, cports[NCLS] = {0, 0, 0}, pin = 0, pout = 0;
  if (vapx_ingest_pair_ports(g_front, ports, 3) != 3 || vapx_ingest_class_ports(g_front, cports, NCLS) != NCLS) return 2;
  ports[3] = cports[2];
  vapx_ingest_ports(g_front, &pin, &pout);
  std::atomic<long> wrong{0}, answered{0};
  // ---- phase 1: PER dialogues per port, connected port by port (slots p * PER ..), every frame answered with its own two echo sizes ----
  std::vector<int> fin(S), fout(S), on(S);
  for (int i = 0; i < S; ++i) { on[i] = i / PER; fin[i] = dial(ports[on[i]]); usleep(20000); }   // one after another: dialogue i takes slot i
  for (int i = 0; i < S; ++i) { fout[i] = dial(pout); usleep(5000); }                            // the k-th output connection listens to the k-th stream
  usleep(100000);
  {
    std::vector<std::thread> th;
    for (int i = 0; i < S; ++i) {
      th.emplace_back([&, i] { send_frames(fin[i], on[i], FRAMES, kPiece[i % 4]); });
      th.emplace_back([&, i] { answered.fetch_add(read_results(fout[i], FRAMES, on[i], &wrong)); });
    }
    for (auto& t : th) t.join();
  }
  if (answered.load() != (long)S * FRAMES || wrong.load() || g_bad_blocks.load()) {
    fprintf(stderr, "phase 1: answered %ld of %d, %ld with wrong echo sizes or classes, %ld packed blocks with a row at a wrong offset\n", answered.load(),
            S * FRAMES, wrong.load(), g_bad_blocks.load());
    return 4;
  }
  // ---- phase 2: churn across ports - every other dialogue dies in the middle of a frame (and of a sample) and comes back on the NEXT port ----
  for (int round = 0; round < 3; ++round) {
    for (int i = round % 2; i < S; i += 2) {   // one at a time: the freed slot is the only free one, the dialogue returns to it
      send_frames(fin[i], on[i], 1, kPiece[i % 4], 1003 + 100 * round);   // a part of a frame, then gone: nothing of it is ever answered
      close(fin[i]);
      usleep(20000);
      on[i] = (on[i] + 1) % NPORT;
      fin[i] = dial(ports[on[i]]);
      usleep(20000);
    }
    std::vector<std::thread> t2;
    answered.store(0);
    for (int i = 0; i < S; ++i) {
      t2.emplace_back([&, i] { send_frames(fin[i], on[i], 5, kPiece[(i + round) % 4]); });
      t2.emplace_back([&, i] { answered.fetch_add(read_results(fout[i], 5, on[i], &wrong)); });
    }
    for (auto& t : t2) t.join();
    if (answered.load() != (long)S * 5 || wrong.load() || g_bad_blocks.load()) {
      fprintf(stderr, "phase 2 round %d: answered %ld of %d, %ld wrong, %ld bad blocks\n", round, answered.load(), S * 5, wrong.load(), g_bad_blocks.load());
      return 5;
    }
  }
  // ---- phase 3: close while a third of the senders are still pushing ----
  std::atomic<bool> stop{false};
  std::vector<std::thread> t4;
  for (int i = 0; i < S; i += 3) t4.emplace_back([&, i] { while (!stop.load()) send_frames(fin[i], on[i], 2, kPiece[i % 4]); });
  usleep(100000);
  vapx_ingest_stats st;
  vapx_ingest_stats_read(g_front, &st, 1);
  vapx_ingest_close(g_front);
  stop.store(true);
  for (auto& t : t4) t.join();
  for (int fd : fin) close(fd);
  for (int fd : fout) close(fd);
  printf("ok: %d dialogues on 3 pair ports and a class port, steps %ld, frames_done %ld, bad blocks %ld\n", S, g_steps.load(), (long)st.frames_done, g_bad_blocks.load());
  return g_bad_blocks.load() ? 6 : 0;
}
