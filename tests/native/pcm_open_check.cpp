// The native front-end's open against an ENGINE that has an input format (vapx_set_input_format), without a GPU: the front-end
// (vap-realtime_amd/csrc/ingest.cpp) is compiled into this program next to stubs of the engine entry points, the stub engine's format is
// a global.  Checked: vapx_ingest_open / _open_group read the format from the engine, vapx_ingest_config.input_format must be 0 or
// equal to it (refused with a message otherwise), gain with a raw format is refused, a shorter config struct means format 0, and the warm-up
// steps the engine with samples_per_ch = hop on silence of that format.  Built and run by tests/test_pcm.py; prints "ok" or what failed.
#include "../../vap-realtime_amd/csrc/ingest.cpp"

#include <cstdlib>

namespace {
int g_engine_format = VAPX_PCM_F32, g_engine_hz = 16000, g_engine_frame_hz = 20;
int g_steps = 0, g_first_byte = -1, g_spc = 0;
size_t g_record = 0;                       // > 0: vapx_step appends this many bytes per stream of its audio block to g_seen
std::vector<uint8_t> g_seen;
int g_fail = 0;
}  // namespace

#define CHECK(cond) do { if (!(cond)) { ++g_fail; printf("FAIL %s:%d: %s (last open error: %s)\n", __FILE__, __LINE__, #cond, vapx_ingest_last_open_error()); } } while (0)

extern "C" {
void* vapx_host_alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
void vapx_host_free(void* p) { free(p); }
int vapx_get_config(vapx_handle, vapx_config* c) {
  memset(c, 0, sizeof *c);
  c->struct_size = sizeof *c; c->frame_hz = g_engine_frame_hz; c->ctx_frames = 50; c->max_streams = 2; c->max_batch = 2; c->mode = VAPX_MODE_VAP;
  return VAPX_OK;
}
int vapx_reset_stream(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_reset_carry(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_step(vapx_handle, int32_t n, const int32_t*, const float* audio, int32_t spc, float* out, int32_t, void*) {
  if (g_steps++ == 0) { g_first_byte = *(const uint8_t*)audio; g_spc = spc; }
  if (g_record) {
    g_seen.insert(g_seen.end(), (const uint8_t*)audio, (const uint8_t*)audio + (size_t)n * g_record);
    memset(out, 0, (size_t)n * VAPX_OUT_STRIDE * sizeof(float));
  }
  return VAPX_OK;
}
int32_t vapx_bad_slots(vapx_handle, int32_t*, int32_t) { return 0; }
const char* vapx_last_error(vapx_handle) { return "stub"; }
int32_t vapx_get_input_format(vapx_handle) { return g_engine_format; }
int32_t vapx_get_input_rate(vapx_handle) { return g_engine_hz; }
}

namespace {
constexpr int T_HOP = 320;   // 50 Hz
int g_step_bad = 0;

// sample i of channel c, as raw bits: every 16-bit pattern / code comes by
unsigned pattern(int c, int i) { return (unsigned)(i * 131 + c * 7919 + 5); }

int traffic_step(void* user, int32_t n, const int32_t*, const float* audio, float* out) {
  const int fmt = *(const int*)user, bps = fmt == VAPX_PCM_S16 ? 2 : 1;
  static int frame = 0;
  const uint8_t* a = (const uint8_t*)audio;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < T_HOP; ++i) {
      unsigned got = 0;
      memcpy(&got, a + ((size_t)c * T_HOP + i) * bps, bps);
      const unsigned want = pattern(c, (frame % 2) * T_HOP + i) & (bps == 2 ? 0xFFFFu : 0xFFu);
      if (got != want) ++g_step_bad;
    }
  ++frame;
  memset(out, 0, (size_t)n * VAPX_OUT_STRIDE * sizeof(float));
  return 0;
}

int dial(int port) {
  int s = socket(AF_INET, SOCK_STREAM, 0);
  sockaddr_in a;
  memset(&a, 0, sizeof a);
  a.sin_family = AF_INET; a.sin_port = htons((uint16_t)port);
  inet_pton(AF_INET, "127.0.0.1", &a.sin_addr);
  for (int t = 0; t < 200 && connect(s, (sockaddr*)&a, sizeof a) != 0; ++t) usleep(5000);
  int one = 1;
  setsockopt(s, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
  return s;
}

bool traffic(vapx_ingest_handle g, int fmt) {
  const int bps = fmt == VAPX_PCM_S16 ? 2 : 1;
  int pin = 0, pout = 0;
  vapx_ingest_ports(g, &pin, &pout);
  const int fin = dial(pin);
  vapx_ingest_stats st;
  for (int t = 0; t < 400; ++t) { vapx_ingest_stats_read(g, &st, 0); if (st.in_connections == 1) break; usleep(5000); }
  const int fout = dial(pout);
  for (int t = 0; t < 400; ++t) { vapx_ingest_stats_read(g, &st, 0); if (st.out_connections == 1) break; usleep(5000); }
  std::vector<uint8_t> data((size_t)2 * T_HOP * 2 * bps);
  for (int i = 0; i < 2 * T_HOP; ++i)
    for (int c = 0; c < 2; ++c) { const unsigned v = pattern(c, i); memcpy(&data[((size_t)i * 2 + c) * bps], &v, bps); }
  const size_t cuts[] = {0, 1, 3, 2 * (size_t)bps + 1, data.size() / 2 - 1, data.size() / 2 + (size_t)bps, data.size() - 1, data.size()};
  for (size_t k = 0; k + 1 < sizeof cuts / sizeof cuts[0]; ++k) {
    if (send(fin, data.data() + cuts[k], cuts[k + 1] - cuts[k], MSG_NOSIGNAL) < 0) return false;
    usleep(3000);
  }
  timeval tv{10, 0};
  setsockopt(fout, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
  const int16_t* table = fmt == VAPX_PCM_MULAW ? kMulaw : kAlaw;
  bool ok = true;
  for (int f = 0; f < 2 && ok; ++f) {
    const size_t total = 4 + 8 + 2 * (4 + 8 * (size_t)T_HOP) + 3 * (4 + 16);
    std::vector<uint8_t> pk(total);
    size_t have = 0;
    while (have < total) { ssize_t r = recv(fout, pk.data() + have, total - have, 0); if (r <= 0) return false; have += (size_t)r; }
    for (int c = 0; c < 2 && ok; ++c)
      for (int i = 0; i < T_HOP; ++i) {
        double x;
        memcpy(&x, pk.data() + 4 + 8 + 4 + (size_t)c * (4 + 8 * T_HOP) + 8 * (size_t)i, 8);
        const unsigned v = pattern(c, f * T_HOP + i);
        const double want = (fmt == VAPX_PCM_S16 ? (double)(int16_t)(v & 0xFFFFu) : (double)table[v & 0xFFu]) / 32768.0;
        if (x != want) { ok = false; break; }
      }
  }
  close(fin); close(fout);
  return ok && g_step_bad == 0;
}

// A uniform mu-law front-end at 8 kHz (the rate and the format are the stub engine's), 50 Hz frames, 3 frames, one stream, the wire bytes
// cut (0) one byte per send, (1) at seeded random places after a connection that hung up inside its second frame, (2) into whole frames.
// In (0) and (1) the next piece is sent when the front-end has read the last one and SO_RCVLOWAT is off, so the parser is entered once per
// piece.  The engine's step must see exactly the de-interleaved codes; the packets must echo the table's values (tests/test_pcm.py holds
// pcm_tables.h to pcm.py), frame by frame.  The other connection kinds under the same cuttings: tests/test_ingest.py
bool mulaw_8k(vapx_handle engine, vapx_ingest_config cfg, int cutting) {
  constexpr int hop = 160, frames = 3;
  constexpr size_t frame_len = 2 * hop;
  g_engine_format = VAPX_PCM_MULAW; g_engine_hz = 8000; g_engine_frame_hz = 50;
  cfg.input_format = 0; cfg.max_wait_us = 20000;
  if (cutting != 2) setenv("VAPX_INGEST_NO_LOWAT", "1", 1);
  vapx_ingest_handle g = nullptr;
  const int rc = vapx_ingest_open(engine, &cfg, &g);
  unsetenv("VAPX_INGEST_NO_LOWAT");
  g_engine_format = VAPX_PCM_F32; g_engine_hz = 16000; g_engine_frame_hz = 20;
  if (rc != VAPX_OK || !g) return false;
  g_seen.clear(); g_record = frame_len;
  int pin = 0, pout = 0;
  vapx_ingest_ports(g, &pin, &pout);
  vapx_ingest_stats st;
  auto wait_in = [&](int64_t want) { for (int t = 0; t < 2000; ++t) { vapx_ingest_stats_read(g, &st, 0); if (st.in_connections == want) return; usleep(1000); } };
  const int fout = dial(pout);
  for (int t = 0; t < 2000; ++t) { vapx_ingest_stats_read(g, &st, 0); if (st.out_connections == 1) break; usleep(1000); }
  unsigned seed = 12345u + (unsigned)cutting;
  auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  int64_t sent = 0;
  bool ok = true;
  auto push = [&](int fd, const std::vector<uint8_t>& data, size_t n_bytes) {
    static const size_t sizes[] = {1, 2, 3, 5, 8, 13, 100, 333};
    for (size_t at = 0; at < n_bytes && ok;) {
      const size_t n = std::min(n_bytes - at, cutting == 0 ? (size_t)1 : cutting == 1 ? sizes[rnd() % 8] : frame_len);
      if (send(fd, data.data() + at, n, MSG_NOSIGNAL) != (ssize_t)n) { ok = false; return; }
      at += n; sent += (int64_t)n;
      for (int spin = 0; cutting != 2; ++spin) {
        vapx_ingest_stats_read(g, &st, 0);
        if (st.rx_bytes == sent) break;
        if (spin > 50000000) { ok = false; return; }
      }
    }
  };
  auto codes = [&](int n_frames, int salt) {   // interleaved (ch1, ch2) codes: every code comes by
    std::vector<uint8_t> d(n_frames * frame_len);
    for (size_t i = 0; i < d.size(); ++i) d[i] = (uint8_t)pattern((int)(i & 1), (int)(i / 2) + salt);
    return d;
  };
  std::vector<std::vector<uint8_t>> expect;   // per answered frame: its wire bytes
  timeval tv{10, 0};
  setsockopt(fout, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
  const size_t total = 4 + 8 + 2 * (4 + 8 * (size_t)hop) + 3 * (4 + 16);
  std::vector<uint8_t> pks((frames + 1) * total);
  size_t have = 0;
  auto read_packets = [&](size_t upto) {      // until `upto` packets are in pks
    while (have < upto * total && ok) {
      const ssize_t r = recv(fout, pks.data() + have, upto * total - have, 0);
      if (r <= 0) ok = false; else have += (size_t)r;
    }
  };
  if (cutting == 1) {
    const std::vector<uint8_t> y = codes(2, 77);
    const int f0 = dial(pin);
    wait_in(1);
    push(f0, y, frame_len + frame_len / 2 + 3);
    read_packets(1);   // its whole frame is answered first: a frame still queued when its connection ends is dropped
    close(f0);
    wait_in(0);
    expect.emplace_back(y.begin(), y.begin() + frame_len);
  }
  const std::vector<uint8_t> x = codes(frames, 0);
  const int fin = dial(pin);
  wait_in(1);
  push(fin, x, x.size());
  for (int f = 0; f < frames; ++f) expect.emplace_back(x.begin() + f * frame_len, x.begin() + (f + 1) * frame_len);
  read_packets(expect.size());   // every packet first: the last one is sent after the last step, g_seen is at rest then
  if (g_seen.size() != expect.size() * frame_len) ok = false;
  for (size_t k = 0; k < expect.size() && ok; ++k) {
    const uint8_t* pk = pks.data() + k * total;
    for (int c = 0; c < 2 && ok; ++c) {
      uint32_t n = 0;
      memcpy(&n, pk + 4 + 8 + (size_t)c * (4 + 8 * hop), 4);
      if (n != (uint32_t)hop) ok = false;
      for (int i = 0; i < hop && ok; ++i) {
        double v;
        memcpy(&v, pk + 4 + 8 + 4 + (size_t)c * (4 + 8 * hop) + 8 * (size_t)i, 8);
        const uint8_t code = expect[k][2 * (size_t)i + c];
        if (v != (double)kMulaw[code] / 32768.0) ok = false;
        if (g_seen[k * frame_len + (size_t)c * hop + i] != code) ok = false;   // the staged block: [2][hop]
      }
    }
  }
  close(fin); close(fout);
  vapx_ingest_close(g);
  g_record = 0;
  return ok;
}
}  // namespace

int main() {
  vapx_handle engine = (vapx_handle)&g_engine_format;   // never dereferenced: every engine call is a stub
  vapx_ingest_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg;
  cfg.gain = 1.0;
  vapx_ingest_handle g = nullptr;

  // the engine's format is taken when the config leaves it 0, and when it names the same one
  for (int fmt : {VAPX_PCM_F32, VAPX_PCM_S16, VAPX_PCM_MULAW, VAPX_PCM_ALAW}) {
    for (int same = 0; same < 2; ++same) {
      g_engine_format = fmt; g_steps = 0;
      cfg.input_format = same ? fmt : 0;
      g = nullptr;
      CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_OK && g != nullptr);
      if (!g) continue;
      const InGeo& q = g->geo[0];                                                        // the one class of a front-end without a table
      CHECK(!g->cls_table && g->n_cls == 1 && g->n_in == 1 && vapx_ingest_class_ports(g, nullptr, 0) == 0 && vapx_ingest_pair_ports(g, nullptr, 0) == 0);
      CHECK(q.fmt == fmt && q.bps() == (fmt == VAPX_PCM_F32 ? 4 : fmt == VAPX_PCM_S16 ? 2 : 1));
      CHECK(2 * q.wire_bps() == (fmt == VAPX_PCM_F32 ? 16 : fmt == VAPX_PCM_S16 ? 4 : 2) && q.hop == 800);
      CHECK(g_steps == 3 && g_spc == 800);                                               // the warm-up, on silence of the format
      CHECK(g_first_byte == (fmt == VAPX_PCM_MULAW ? 0xFF : fmt == VAPX_PCM_ALAW ? 0xD5 : 0));
      CHECK((fmt == VAPX_PCM_F32) == !g->echo.empty());                                  // no f64 copy per slot with a raw format
      vapx_ingest_close(g);
    }
  }
  // a config format that disagrees with the engine's
  g_engine_format = VAPX_PCM_S16; cfg.input_format = VAPX_PCM_MULAW; g = nullptr;
  CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_E_INVAL && g == nullptr);
  CHECK(strstr(vapx_ingest_last_open_error(), "differs from the engine's input format") != nullptr);
  g_engine_format = VAPX_PCM_F32; cfg.input_format = VAPX_PCM_ALAW; g = nullptr;
  CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_E_INVAL && strstr(vapx_ingest_last_open_error(), "differs from the engine's") != nullptr);
  // an unknown id
  cfg.input_format = 4; g = nullptr;
  CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_E_INVAL && strstr(vapx_ingest_last_open_error(), "input_format: known are") != nullptr);
  // gain with a raw format (read from the engine)
  g_engine_format = VAPX_PCM_MULAW; cfg.input_format = 0; cfg.gain = 2.0; g = nullptr;
  CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_E_INVAL && strstr(vapx_ingest_last_open_error(), "gain with a raw input format") != nullptr);
  g_engine_format = VAPX_PCM_F32; g = nullptr;
  CHECK(vapx_ingest_open(engine, &cfg, &g) == VAPX_OK);                                  // gain and f64 framing: as ever
  if (g) { CHECK(g->geo[0].fmt == VAPX_PCM_F32 && g->cfg.gain == 2.0); vapx_ingest_close(g); }
  cfg.gain = 1.0;
  // the struct as it was before the field: format 0, whatever lies behind it
  cfg.input_format = VAPX_PCM_S16;
  cfg.struct_size = (int32_t)offsetof(vapx_ingest_config, input_format);
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->geo[0].fmt == VAPX_PCM_F32); vapx_ingest_close(g); }
  cfg.struct_size = (int32_t)offsetof(vapx_ingest_config, cpu_first);
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->geo[0].fmt == VAPX_PCM_F32); vapx_ingest_close(g); }
  cfg.struct_size = sizeof cfg;
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->geo[0].fmt == VAPX_PCM_S16 && g->echo.empty()); vapx_ingest_close(g); }
  // traffic in each raw format over a step function: two frames in chunks that split sample pairs and cross the frame boundary; the step
  // sees the de-interleaved samples, the result packets echo their values (tests/test_pcm.py builds this program with -fsanitize=address,undefined: this walks every
  // offset of the raw staging)
  for (int fmt : {VAPX_PCM_S16, VAPX_PCM_MULAW, VAPX_PCM_ALAW}) {
    cfg.input_format = fmt; cfg.max_wait_us = 200000;
    g = nullptr;
    CHECK(vapx_ingest_open_fn(traffic_step, nullptr, &fmt, 1, 1, 50, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
    if (!g) continue;
    CHECK(traffic(g, fmt));
    vapx_ingest_close(g);
  }
  for (int cutting = 0; cutting < 3; ++cutting) CHECK(mulaw_8k(engine, cfg, cutting));
  if (g_fail == 0) printf("ok\n");
  return g_fail ? 1 : 0;
}
