// Host cost of the native front-end's frame parser per wire byte, without a GPU and without sockets: the front-end
// (vap-realtime_amd/csrc/ingest.cpp) is compiled INTO this program next to stubs of the engine entry points, as the tests/native
// programs are, and main() drives feed() on slot 0 with pre-built wire bytes in 10 ms packets.  The step returns at once; when no
// frame buffer is free main waits for the tick and sender threads, and that wait is not timed.
//
//   g++ -O2 -std=c++17 -pthread -Wno-subobject-linkage [-DINGEST_CPP='"/path/to/another/ingest.cpp"'] tools/frontend_feed_bench.cpp -o tools/frontend_feed_bench
//   tools/frontend_feed_bench [--seconds 1.0] [--core N] [--frame-hz 20]     one JSON line: ns per wire byte of every leg
//
// Every complete frame costs one hand-over to the tick thread (a mutex and a condition-variable wake-up), which is not the parser: at
// --frame-hz 5 a frame holds four times the bytes of one at 20, and the figure is that much closer to the parser's own cost.
//
// --core N: the feeding thread sits on core N, the front-end's threads on cores N+1 .. N+3 (vapx_ingest_config.cpu_first / cpu_count).
// tools/frontend_feed_ab.py builds this against two trees and runs them alternately.
#ifndef INGEST_CPP
#define INGEST_CPP "../vap-realtime_amd/csrc/ingest.cpp"
#endif
#include INGEST_CPP

#include <cstdlib>
#include <random>

namespace {
int g_engine_format = VAPX_PCM_F32, g_engine_hz = 16000, g_frame_hz = 20;
}

extern "C" {
void* vapx_host_alloc(size_t bytes) { return calloc(1, bytes ? bytes : 1); }
void vapx_host_free(void* p) { free(p); }
int vapx_get_config(vapx_handle, vapx_config* c) {
  memset(c, 0, sizeof *c);
  c->struct_size = sizeof *c; c->frame_hz = g_frame_hz; c->ctx_frames = 50; c->max_streams = 1; c->max_batch = 1; c->mode = VAPX_MODE_VAP;
  return VAPX_OK;
}
int vapx_reset_stream(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_reset_carry(vapx_handle, int32_t) { return VAPX_OK; }
int vapx_step(vapx_handle, int32_t, const int32_t*, const float*, int32_t, float*, int32_t, void*) { return VAPX_OK; }
int32_t vapx_bad_slots(vapx_handle, int32_t*, int32_t) { return 0; }
const char* vapx_last_error(vapx_handle) { return "stub"; }
int32_t vapx_get_input_format(vapx_handle) { return g_engine_format; }
int32_t vapx_get_input_rate(vapx_handle) { return g_engine_hz; }
}

namespace {
int step_at_once(void*, int32_t, const int32_t*, const float*, float*) { return 0; }

// `packets`: one frame's wire bytes, cut into its 10 ms packets.  Feeds frames until `seconds` of feed() time are spent
double run_leg(vapx_ingest* g, const std::vector<std::vector<uint8_t>>& packets, double seconds) {
  double spent = 0.0;
  int64_t bytes = 0;
  while (spent < seconds) {
    double t0 = mono_now();
    for (int rep = 0; rep < 64; ++rep)
      for (const auto& pk : packets) {
        size_t at = 0;
        for (;;) {
          at += feed(g, 0, pk.data() + at, pk.size() - at);
          if (at == pk.size()) break;
          spent += mono_now() - t0;                   // no frame buffer is free: wait for the tick and the senders, untimed
          while (std::none_of(g->slots[0].state, g->slots[0].state + NBUF, [](std::atomic<int>& b) { return b.load() == B_FREE; })) std::this_thread::yield();
          t0 = mono_now();
        }
        bytes += (int64_t)pk.size();
      }
    spent += mono_now() - t0;
  }
  return spent * 1e9 / (double)bytes;
}

std::vector<std::vector<uint8_t>> cut(const std::vector<uint8_t>& frame, int n_packets) {
  std::vector<std::vector<uint8_t>> pk;
  const size_t each = frame.size() / n_packets;
  for (int k = 0; k < n_packets; ++k) pk.emplace_back(frame.begin() + k * each, frame.begin() + (k + 1) * each);
  return pk;
}
}  // namespace

int main(int argc, char** argv) {
  double seconds = 1.0;
  int core = -1;
  for (int i = 1; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--seconds")) seconds = atof(argv[i + 1]);
    else if (!strcmp(argv[i], "--core")) core = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--frame-hz")) g_frame_hz = atoi(argv[i + 1]);
  }
  if (core >= 0) {
    cpu_set_t set;
    CPU_ZERO(&set); CPU_SET(core, &set);
    sched_setaffinity(0, sizeof set, &set);
  }
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  auto f64_bytes = [&](size_t n) { std::vector<uint8_t> b(8 * n); for (size_t i = 0; i < n; ++i) { const double v = u(rng); memcpy(&b[8 * i], &v, 8); } return b; };
  auto raw_bytes = [&](size_t n) { std::vector<uint8_t> b(n); for (auto& x : b) x = (uint8_t)rng(); return b; };

  vapx_handle engine = (vapx_handle)&g_engine_format;   // never dereferenced: every engine call is a stub
  printf("{");
  struct Leg { const char* name; int fmt, hz; double gain; bool pair; };
  const std::string f64 = "f64_" + std::to_string(g_frame_hz) + "hz_gain", g1 = f64 + "1", g2 = f64 + "2";
  const Leg legs[] = {{g1.c_str(), VAPX_PCM_F32, 16000, 1.0, false}, {g2.c_str(), VAPX_PCM_F32, 16000, 2.0, false},
                      {"s16_16k", VAPX_PCM_S16, 16000, 1.0, false}, {"mulaw_8k", VAPX_PCM_MULAW, 8000, 1.0, false},
                      {"pair_f64_16k_mulaw_8k", 0, 0, 1.0, true}};
  bool first = true;
  for (const Leg& leg : legs) {
    vapx_ingest_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.gain = leg.gain;
    cfg.port_in = cfg.port_out = -1;        // passive: no listen sockets, no accept thread; slot 0 is fed from here
    cfg.max_wait_us = 100;
    cfg.flags = VAPX_INGEST_KEEP_NOFILE;
    if (core >= 0) { cfg.cpu_first = core + 1; cfg.cpu_count = 3; }
    vapx_ingest_handle g = nullptr;
    std::vector<std::vector<uint8_t>> packets;
    const int hz = g_frame_hz, pk = 100 / hz;
    int rc;
    if (leg.pair) {   // a pair port's stream: planar packets, channel 1 f64 at 16 kHz, channel 2 mu-law at 8 kHz
      cfg.port_in = cfg.port_out = 0;       // (a table's front-end is never passive: it listens on ephemeral ports nobody dials)
      cfg.n_input_classes = 2;
      cfg.input_classes[0] = {16000, VAPX_PCM_F32};
      cfg.input_classes[1] = {8000, VAPX_PCM_MULAW};
      cfg.n_pair_ports = 1;
      cfg.pair_ports[0].cls_ch1 = 0; cfg.pair_ports[0].cls_ch2 = 1; cfg.pair_ports[0].port_in = 0;
      rc = vapx_ingest_open_fn(step_at_once, nullptr, nullptr, 1, 1, hz, VAPX_MODE_VAP, &cfg, &g);
      if (rc == VAPX_OK) {
        Slot& s = g->slots[0];              // what adopting a connection of that port writes
        s.cls = 0; s.cls2 = 1; s.planar = true;
        for (int k = 0; k < pk; ++k) {
          std::vector<uint8_t> p = f64_bytes(160), c2 = raw_bytes(80);
          p.insert(p.end(), c2.begin(), c2.end());
          packets.push_back(p);
        }
      }
    } else {
      g_engine_format = leg.fmt; g_engine_hz = leg.hz;
      cfg.flags |= VAPX_INGEST_KEEP_STATE;
      rc = vapx_ingest_open(engine, &cfg, &g);
      const size_t pairs = (size_t)leg.hz / hz;
      if (rc == VAPX_OK) packets = cut(leg.fmt == VAPX_PCM_F32 ? f64_bytes(2 * pairs) : raw_bytes(2 * pairs * (leg.fmt == VAPX_PCM_S16 ? 2 : 1)), pk);
    }
    if (rc != VAPX_OK) { fprintf(stderr, "open failed for %s: %d %s\n", leg.name, rc, vapx_ingest_last_open_error()); return 1; }
    run_leg(g, packets, 0.05);              // warm the caches and the threads
    const double ns = run_leg(g, packets, seconds);
    printf("%s\"%s\": %.4f", first ? "" : ", ", leg.name, ns);
    first = false;
    vapx_ingest_close(g);
  }
  printf("}\n");
  return 0;
}
