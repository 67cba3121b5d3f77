// The engine's buffer table (csrc/engine_buffers.h) against the sizes written out by hand, and Scratch::slice against the table:
// for every geometry, window, batch and number of overlap groups, group g's slice of every buffer starts b0 x (elements per slot) into
// it, consecutive groups abut and the last one ends exactly at the allocated size.  Plain C++, built with ASan + UBSan by
// tests/test_engine_buffers.py.  The buffers are address space only (PROT_NONE mappings of the largest size): nothing is read or written.
// Then vapx_peek's refusal rules (peek_refusal, ring_direct_for, prune_last_for of the same header) against a table written out by hand.
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

// vapx_peek's rules (peek_refusal and the two create-time decisions it is given) against the answers written out by hand.  0 = readable
static void check_peek_rules() {
  const char* const OK = nullptr;
  const char *PRE = kPeekNotInPrefill, *LDS = kPeekInLds, *X0 = kPeekX0InRing, *S2 = kPeekStereo2Pruned, *LAST = kPeekLastEveryRow,
             *NOD = kPeekCombNotNod, *SPLIT = kPeekCombSplit;
  // every peek name after a step, after a prefill chunk and after either with the fused conv tail: a default engine (vap, the rings read
  // in place, the last layer on the newest row), one group
  const PassRecord step{64, 1, false, false}, prefill{40, 1, true, false}, step_tail{64, 1, false, true}, prefill_tail{40, 1, true, true};
  const struct { const char* name; const char *step, *prefill, *step_tail, *prefill_tail; } by_pass[] = {
      {"h0", OK, OK, OK, OK},         {"h1", OK, OK, OK, OK},         {"h2", OK, OK, LDS, LDS},       {"h3", OK, OK, LDS, LDS},
      {"z", OK, OK, OK, OK},          {"lstm_out", OK, PRE, OK, PRE}, {"e", OK, OK, OK, OK},          {"x0", X0, PRE, X0, PRE},
      {"o", OK, PRE, OK, PRE},        {"stereo0", OK, PRE, OK, PRE},  {"stereo1", OK, PRE, OK, PRE},  {"stereo2", S2, PRE, S2, PRE},
      {"last", OK, PRE, OK, PRE},     {"comb", NOD, PRE, NOD, PRE},
  };
  size_t named = 0;
  for (const ScratchRow& r : kScratchTable) named += r.peek != nullptr;
  CHECK(named == sizeof by_pass / sizeof by_pass[0], "%zu peek names in the table, %zu in the hand-written list", named, sizeof by_pass / sizeof by_pass[0]);
  for (const auto& c : by_pass) {
    CHECK(scratch_row_by_peek(c.name) != nullptr, "%s is no peek name", c.name);
    CHECK(peek_refusal(step, VAPX_MODE_VAP, true, true, false, c.name) == c.step, "%s after a step", c.name);
    CHECK(peek_refusal(prefill, VAPX_MODE_VAP, true, true, false, c.name) == c.prefill, "%s after a prefill", c.name);
    CHECK(peek_refusal(step_tail, VAPX_MODE_VAP, true, true, false, c.name) == c.step_tail, "%s after a step with the fused tail", c.name);
    CHECK(peek_refusal(prefill_tail, VAPX_MODE_VAP, true, true, false, c.name) == c.prefill_tail, "%s after a prefill with the fused tail", c.name);
  }
  // "x0": the window either side of the short-window block's limit x the two flags that decide
  const struct { int T, flags; bool ring_direct; } x0s[] = {
      {64, 0, true},  {64, VAPX_FLAG_UNFUSED_PROJ, true},  {64, VAPX_FLAG_MATERIALIZE_X0, false},
      {65, 0, true},  {65, VAPX_FLAG_UNFUSED_PROJ, false}, {65, VAPX_FLAG_MATERIALIZE_X0, false},
  };
  for (const auto& c : x0s) {
    CHECK(ring_direct_for(c.flags, c.T) == c.ring_direct, "ring_direct at T = %d, flags 0x%x", c.T, c.flags);
    CHECK(peek_refusal(step, VAPX_MODE_VAP, ring_direct_for(c.flags, c.T), true, false, "x0") == (c.ring_direct ? X0 : OK), "x0 at T = %d, flags 0x%x", c.T, c.flags);
  }
  // the last layer: vap / nod x VAPX_FLAG_FULL_LAST_LAYER
  const struct { int mode, flags; bool prune; const char *stereo2, *last, *comb; } lasts[] = {
      {VAPX_MODE_VAP, 0, true, S2, OK, NOD},  {VAPX_MODE_VAP, VAPX_FLAG_FULL_LAST_LAYER, false, OK, LAST, NOD},
      {VAPX_MODE_NOD, 0, false, OK, LAST, OK}, {VAPX_MODE_NOD, VAPX_FLAG_FULL_LAST_LAYER, false, OK, LAST, OK},
  };
  for (const auto& c : lasts) {
    const bool prune = prune_last_for(c.flags, c.mode);
    CHECK(prune == c.prune, "prune_last in mode %d, flags 0x%x", c.mode, c.flags);
    CHECK(peek_refusal(step, c.mode, true, prune, false, "stereo2") == c.stereo2, "stereo2 in mode %d, flags 0x%x", c.mode, c.flags);
    CHECK(peek_refusal(step, c.mode, true, prune, false, "last") == c.last, "last in mode %d, flags 0x%x", c.mode, c.flags);
    CHECK(peek_refusal(step, c.mode, true, prune, false, "comb") == c.comb, "comb in mode %d, flags 0x%x", c.mode, c.flags);
  }
  CHECK(prune_last_for(0, VAPX_MODE_BC), "bc prunes the last layer");
  // "comb" in one and in two overlap groups; a released encoder buffer; a name the table does not have
  const PassRecord two_groups{64, 2, false, false};
  CHECK(peek_refusal(step, VAPX_MODE_NOD, true, false, false, "comb") == OK, "comb in one group");
  CHECK(peek_refusal(two_groups, VAPX_MODE_NOD, true, false, false, "comb") == SPLIT, "comb in two groups");
  CHECK(peek_refusal(two_groups, VAPX_MODE_NOD, true, false, false, "o") == OK, "o in two groups");
  CHECK(peek_refusal(step, VAPX_MODE_VAP, true, true, true, "h0") == kPeekReleased, "a released h0");
  CHECK(peek_refusal(prefill, VAPX_MODE_VAP, true, true, true, "lstm_out") == PRE, "a released lstm_out after a prefill: the prefill's rule comes first");
  CHECK(peek_refusal(step, VAPX_MODE_VAP, true, true, false, "qkv") == kPeekUnknown, "a buffer without a peek name");
  CHECK(strstr(kPeekCombSplit, "%d") && !strstr(kPeekCombSplit, "%s"), "the one format that takes the group count");
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
  check_peek_rules();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok: %zu buffers, %ld slices\n", sizeof kScratchTable / sizeof kScratchTable[0], shapes);
  return 0;
}
