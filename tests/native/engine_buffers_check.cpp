// The engine's buffer table (csrc/engine_buffers.h) against the sizes written out by hand, and Scratch::slice against the table:
// for every geometry, window, batch and number of overlap groups, group g's slice of every buffer starts b0 x (elements per slot) into
// it, consecutive groups abut and the last one ends exactly at the allocated size.  Plain C++, built with ASan + UBSan by
// tests/test_engine_buffers.py.  The buffers are address space only (PROT_NONE mappings of the largest size): nothing is read or written.
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "../../vap-realtime_amd/csrc/engine_buffers.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// elements per batch slot, as vapx_create allocated them before the table existed
static std::map<std::string, size_t> expected_sizes(const int* P, int ncpc, int T) {
  std::map<std::string, size_t> m;
  m["out_dev"] = VAPX_OUT_STRIDE;
  m["bn"] = m["bhead"] = m["rot"] = 1;
  m["h0"] = (size_t)2 * (P[0] + 4) * 256;
  m["h1"] = (size_t)2 * (P[1] + 2) * 256;
  m["h2"] = (size_t)2 * (P[2] + 2) * 256;
  m["h3"] = (size_t)2 * (P[3] + 2) * 256;
  m["z"] = m["lstm_out"] = (size_t)2 * ncpc * 256;
  m["gx"] = (size_t)2 * ncpc * 1024;
  m["e"] = m["en"] = 512;
  for (const char* n : {"xl[0]", "xl[1]", "xl[2]", "xl[3]", "xl[4]", "xn", "xmid", "att", "qx"}) m[n] = (size_t)2 * T * 256;
  m["kvx"] = (size_t)2 * T * 512;
  m["qkv"] = (size_t)2 * T * 768;
  for (const char* n : {"last[0]", "last[1]", "last[2]", "last[3]", "last[4]", "last[5]"}) m[n] = 512;
  m["qkv_new"] = m["lffn"] = 1536;
  return m;
}

int main() {
  const std::set<std::string> want_poison = {"z", "gx", "lstm_out", "e", "xl[0]", "xl[1]", "xl[2]", "xl[3]", "xl[4]", "xn", "xmid", "att", "qkv", "qx",
                                             "kvx", "last[0]", "last[1]", "last[2]", "last[3]", "last[4]", "last[5]", "en", "qkv_new", "lffn", "out_dev"};
  const std::set<std::string> want_release = {"h0", "h1", "h2", "h3", "z", "gx", "lstm_out"};
  const std::map<std::string, std::string> want_peek = {{"h0", "h0"}, {"h1", "h1"}, {"h2", "h2"}, {"h3", "h3"}, {"z", "z"}, {"lstm_out", "lstm_out"},
      {"e", "e"}, {"xl[0]", "x0"}, {"xl[1]", "o"}, {"xl[2]", "stereo0"}, {"xl[3]", "stereo1"}, {"xl[4]", "stereo2"}, {"last[5]", "last"}, {"xmid", "comb"}};
  std::set<std::string> poison, release, members;
  std::map<std::string, std::string> peek;
  for (const ScratchRow& r : kScratchTable) {
    CHECK(members.insert(r.member).second, "%s appears twice", r.member);
    if (r.poison) poison.insert(r.member);
    if (r.encoder) release.insert(r.member);
    if (r.peek) {
      peek[r.member] = r.peek;
      CHECK(scratch_row_by_peek(r.peek) == &r, "peek name %s does not find its row", r.peek);
    }
  }
  CHECK(poison == want_poison, "the poison set has %zu members", poison.size());
  CHECK(release == want_release, "the follower-release set has %zu members", release.size());
  CHECK(peek == want_peek, "the peek names differ");
  CHECK(scratch_row_by_peek("qkv") == nullptr, "a buffer without a peek name was found");

  // geometry: 16 kHz frames with 320 samples of carry through strides 5, 4, 2, 2, 2
  const int hzs[] = {5, 10, 20, 50}, Ts[] = {1, 64, 65, 250, 512}, Bs[] = {1, 77, 1000};
  const int want_P[4][5] = {{704, 176, 88, 44, 22}, {384, 96, 48, 24, 12}, {224, 56, 28, 14, 7}, {128, 32, 16, 8, 4}};
  const size_t maxB = 1000;
  std::map<std::string, size_t> cap;   // largest allocation over all shapes, in elements
  for (int hz : hzs) {
    const auto m = expected_sizes(geometry(hz, 512).P, geometry(hz, 512).ncpc, 512);
    for (const auto& kv : m) cap[kv.first] = std::max(cap[kv.first], kv.second * maxB);
  }
  Scratch base;
  for (const ScratchRow& r : kScratchTable) {
    CHECK(cap.count(r.member) == 1, "no expected size for %s", r.member);
    void* p = mmap(nullptr, cap[r.member] * 4, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) { printf("mmap of %zu bytes failed\n", cap[r.member] * 4); return 2; }
    const ScratchSlot s = r.slot(base);
    CHECK((s.f != nullptr) != (s.i != nullptr), "%s: exactly one of the two slots", r.member);
    if (s.f) *s.f = (float*)p; else *s.i = (int*)p;
  }
  CHECK(cap.size() == sizeof kScratchTable / sizeof kScratchTable[0], "%zu expected sizes, %zu rows", cap.size(), sizeof kScratchTable / sizeof kScratchTable[0]);

  long shapes = 0;
  for (int hi = 0; hi < 4; ++hi)
    for (int T : Ts) {
      const Geometry geo = geometry(hzs[hi], T);
      CHECK(geo.hop == 16000 / hzs[hi] && geo.L == geo.hop + 320 && geo.T == T && geo.ncpc == want_P[hi][4] - 2, "geometry at %d Hz", hzs[hi]);
      for (int i = 0; i < 5; ++i) CHECK(geo.P[i] == want_P[hi][i], "P[%d] at %d Hz = %d", i, hzs[hi], geo.P[i]);
      const auto want = expected_sizes(want_P[hi], want_P[hi][4] - 2, T);
      for (const ScratchRow& r : kScratchTable)
        CHECK(r.per_slot(geo) == want.at(r.member), "%s at %d Hz, T = %d: %zu per slot, expected %zu", r.member, hzs[hi], T, r.per_slot(geo), want.at(r.member));
      for (int B : Bs)
        for (int G = 1; G <= 8; ++G) {
          Scratch prev;
          for (int g = 0; g <= G; ++g) {   // g == G: the end of the last group, i.e. of the allocation
            const size_t b0 = (size_t)((long)B * g / G);
            Scratch cur = base.slice(b0, geo);
            for (const ScratchRow& r : kScratchTable) {
              const size_t per = want.at(r.member);
              const uintptr_t at = (uintptr_t)scratch_ptr(r, cur), start = (uintptr_t)scratch_ptr(r, base);
              CHECK(at - start == b0 * per * 4, "%s: slice at b0 = %zu starts %zu bytes in, expected %zu", r.member, b0, (size_t)(at - start), b0 * per * 4);
              if (g > 0) {   // group g - 1 holds nb slots from its own start: it ends where group g (or the allocation) begins
                const size_t nb = b0 - (size_t)((long)B * (g - 1) / G);
                CHECK((uintptr_t)scratch_ptr(r, prev) + nb * per * 4 == at, "%s: groups %d and %d of %d do not abut (B = %d)", r.member, g - 1, g, G, B);
              }
              if (g == G) CHECK(at - start == (size_t)B * per * 4, "%s: the last group does not end at the allocated size", r.member);
            }
            prev = cur;
            ++shapes;
          }
        }
    }
  // a released buffer stays null in every slice
  Scratch rel = base;
  rel.h2 = nullptr; rel.bn = nullptr;
  const Scratch rs = rel.slice(5, geometry(20, 50));
  CHECK(rs.h2 == nullptr && rs.bn == nullptr && rs.h1 == base.h1 + (size_t)5 * 2 * (56 + 2) * 256, "slice of a released buffer");
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok: %zu buffers, %ld slices\n", sizeof kScratchTable / sizeof kScratchTable[0], shapes);
  return 0;
}
