// The native front-end's open against an ENGINE that has an input format (vapx_set_input_format), without a GPU: the front-end
// (vap-realtime_amd/csrc/ingest.cpp) is compiled into this program next to stubs of the engine entry points, the stub engine's format is
// a global.  Checked: vapx_ingest_open / _open_group read the format from the engine, vapx_ingest_config.input_format must be 0 or
// equal to it (refused with a message otherwise), gain with a raw format is refused, a shorter config struct means format 0, and the warm-up
// steps the engine with samples_per_ch = hop on silence of that format.  Built and run by tests/test_pcm.py; prints "ok" or what failed.
#include "../../vap-realtime_amd/csrc/ingest.cpp"

#include <cstdlib>

namespace {
int g_engine_format = VAPX_PCM_F32;
int g_steps = 0, g_first_byte = -1, g_spc = 0;
int g_fail = 0;
}  // namespace

#define CHECK(cond) do { if (!(cond)) { ++g_fail; printf("FAIL %s:%d: %s (last open error: %s)\n", __FILE__, __LINE__, #cond, vapx_ingest_last_open_error()); } } while (0)

extern "C" {
void* vapx_host_alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
void vapx_host_free(void* p) { free(p); }
int vapx_get_config(vapx_handle, vapx_config* c) {
  memset(c, 0, sizeof *c);
  c->struct_size = sizeof *c; c->frame_hz = 20; c->ctx_frames = 50; c->max_streams = 2; c->max_batch = 2; c->mode = VAPX_MODE_VAP;
  return VAPX_OK;
}
int vapx_reset_stream(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_reset_carry(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_step(vapx_handle, int32_t, const int32_t*, const float* audio, int32_t spc, float*, int32_t, void*) {
  if (g_steps++ == 0) { g_first_byte = *(const uint8_t*)audio; g_spc = spc; }
  return VAPX_OK;
}
int32_t vapx_bad_slots(vapx_handle, int32_t*, int32_t) { return 0; }
const char* vapx_last_error(vapx_handle) { return "stub"; }
int32_t vapx_get_input_format(vapx_handle) { return g_engine_format; }
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

bool traffic(vapx_ingest_handle g, int fmt) {
  const int bps = fmt == VAPX_PCM_S16 ? 2 : 1;
  int pin = 0, pout = 0;
  vapx_ingest_ports(g, &pin, &pout);
  auto dial = [](int port) {
    int s = socket(AF_INET, SOCK_STREAM, 0);
    sockaddr_in a;
    memset(&a, 0, sizeof a);
    a.sin_family = AF_INET; a.sin_port = htons((uint16_t)port);
    inet_pton(AF_INET, "127.0.0.1", &a.sin_addr);
    for (int t = 0; t < 200 && connect(s, (sockaddr*)&a, sizeof a) != 0; ++t) usleep(5000);
    return s;
  };
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
      CHECK(g->fmt == fmt && g->bps == (fmt == VAPX_PCM_F32 ? 4 : fmt == VAPX_PCM_S16 ? 2 : 1));
      CHECK(g->pair_bytes == (fmt == VAPX_PCM_F32 ? 16 : fmt == VAPX_PCM_S16 ? 4 : 2) && g->hop == 800);
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
  if (g) { CHECK(g->fmt == VAPX_PCM_F32 && g->cfg.gain == 2.0); vapx_ingest_close(g); }
  cfg.gain = 1.0;
  // the struct as it was before the field: format 0, whatever lies behind it
  cfg.input_format = VAPX_PCM_S16;
  cfg.struct_size = (int32_t)offsetof(vapx_ingest_config, input_format);
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->fmt == VAPX_PCM_F32); vapx_ingest_close(g); }
  cfg.struct_size = (int32_t)offsetof(vapx_ingest_config, cpu_first);
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->fmt == VAPX_PCM_F32); vapx_ingest_close(g); }
  cfg.struct_size = sizeof cfg;
  g = nullptr;
  CHECK(vapx_ingest_open_fn([](void*, int32_t, const int32_t*, const float*, float*) { return 0; }, nullptr, nullptr, 2, 2, 20, VAPX_MODE_VAP, &cfg, &g) == VAPX_OK);
  if (g) { CHECK(g->fmt == VAPX_PCM_S16 && g->echo.empty()); vapx_ingest_close(g); }
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
  if (g_fail == 0) printf("ok\n");
  return g_fail ? 1 : 0;
}
