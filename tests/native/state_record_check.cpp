// A stream's state record (csrc/state_record.h) against figures written out by hand: where every section starts for each window, role,
// resampler history and cache choice, and which rule a header offered for import breaks first.  Plain C++, built with ASan + UBSan by
// tests/test_state_record.py.
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../vap-realtime_amd/csrc/state_record.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// header | lstm 1024 | carry 640 | history | ring 2.T.256 | cache 2.T.768, as include/vapx.h lists them
static const struct { int T, with_state, rs_rec, with_cache; long lstm, carry, history, ring, cache, total; } kLayouts[] = {
    // T = 1
    {1, 1, 0, 0, 8, 1032, -1, 1672, -1, 2184},         {1, 1, 0, 1, 8, 1032, -1, 1672, 2184, 3720},
    {1, 1, 28, 0, 8, 1032, 1672, 1700, -1, 2212},      {1, 1, 28, 1, 8, 1032, 1672, 1700, 2212, 3748},
    {1, 1, 56, 0, 8, 1032, 1672, 1728, -1, 2240},      {1, 1, 56, 1, 8, 1032, 1672, 1728, 2240, 3776},
    {1, 1, 80, 0, 8, 1032, 1672, 1752, -1, 2264},      {1, 1, 80, 1, 8, 1032, 1672, 1752, 2264, 3800},
    {1, 0, 0, 0, -1, -1, -1, 8, -1, 520},              {1, 0, 0, 1, -1, -1, -1, 8, 520, 2056},
    {1, 0, 28, 0, -1, -1, 8, 36, -1, 548},             {1, 0, 28, 1, -1, -1, 8, 36, 548, 2084},
    {1, 0, 56, 0, -1, -1, 8, 64, -1, 576},             {1, 0, 56, 1, -1, -1, 8, 64, 576, 2112},
    {1, 0, 80, 0, -1, -1, 8, 88, -1, 600},             {1, 0, 80, 1, -1, -1, 8, 88, 600, 2136},
    // T = 50: ring 25600, cache 76800
    {50, 1, 0, 0, 8, 1032, -1, 1672, -1, 27272},       {50, 1, 0, 1, 8, 1032, -1, 1672, 27272, 104072},
    {50, 1, 28, 0, 8, 1032, 1672, 1700, -1, 27300},    {50, 1, 28, 1, 8, 1032, 1672, 1700, 27300, 104100},
    {50, 1, 56, 0, 8, 1032, 1672, 1728, -1, 27328},    {50, 1, 56, 1, 8, 1032, 1672, 1728, 27328, 104128},
    {50, 1, 80, 0, 8, 1032, 1672, 1752, -1, 27352},    {50, 1, 80, 1, 8, 1032, 1672, 1752, 27352, 104152},
    {50, 0, 0, 0, -1, -1, -1, 8, -1, 25608},           {50, 0, 0, 1, -1, -1, -1, 8, 25608, 102408},
    {50, 0, 28, 0, -1, -1, 8, 36, -1, 25636},          {50, 0, 28, 1, -1, -1, 8, 36, 25636, 102436},
    {50, 0, 56, 0, -1, -1, 8, 64, -1, 25664},          {50, 0, 56, 1, -1, -1, 8, 64, 25664, 102464},
    {50, 0, 80, 0, -1, -1, 8, 88, -1, 25688},          {50, 0, 80, 1, -1, -1, 8, 88, 25688, 102488},
    // T = 512: ring 262144, cache 786432
    {512, 1, 0, 0, 8, 1032, -1, 1672, -1, 263816},     {512, 1, 0, 1, 8, 1032, -1, 1672, 263816, 1050248},
    {512, 1, 28, 0, 8, 1032, 1672, 1700, -1, 263844},  {512, 1, 28, 1, 8, 1032, 1672, 1700, 263844, 1050276},
    {512, 1, 56, 0, 8, 1032, 1672, 1728, -1, 263872},  {512, 1, 56, 1, 8, 1032, 1672, 1728, 263872, 1050304},
    {512, 1, 80, 0, 8, 1032, 1672, 1752, -1, 263896},  {512, 1, 80, 1, 8, 1032, 1672, 1752, 263896, 1050328},
    {512, 0, 0, 0, -1, -1, -1, 8, -1, 262152},         {512, 0, 0, 1, -1, -1, -1, 8, 262152, 1048584},
    {512, 0, 28, 0, -1, -1, 8, 36, -1, 262180},        {512, 0, 28, 1, -1, -1, 8, 36, 262180, 1048612},
    {512, 0, 56, 0, -1, -1, 8, 64, -1, 262208},        {512, 0, 56, 1, -1, -1, 8, 64, 262208, 1048640},
    {512, 0, 80, 0, -1, -1, 8, 88, -1, 262232},        {512, 0, 80, 1, -1, -1, 8, 88, 262232, 1048664},
};

static void check_layouts() {
  for (const auto& w : kLayouts) {
    const StateLayout l = state_layout(w.T, w.with_state != 0, w.rs_rec, w.with_cache != 0);
    const long got[] = {l.header, l.lstm, l.carry, l.history, l.ring, l.cache, l.total};
    const long want[] = {0, w.lstm, w.carry, w.history, w.ring, w.cache, w.total};
    const char* const name[] = {"header", "lstm", "carry", "history", "ring", "cache", "total"};
    long prev = -1;
    for (int i = 0; i < 7; ++i) {
      CHECK(got[i] == want[i], "T = %d, state %d, history %d, cache %d: %s at %ld, expected %ld", w.T, w.with_state, w.rs_rec, w.with_cache, name[i], got[i], want[i]);
      if (got[i] < 0) continue;
      CHECK(got[i] % 4 == 0, "%s at %ld is not 16-byte aligned", name[i], got[i]);
      CHECK(got[i] > prev, "%s at %ld does not follow the section before it (%ld)", name[i], got[i], prev);
      prev = got[i];
    }
    // the formula of include/vapx.h
    const long formula = 8 + (w.with_state ? 1664 : 0) + w.rs_rec + 2L * w.T * 256 + (w.with_cache ? 2L * w.T * 768 : 0);
    CHECK(l.total == formula, "T = %d: total %ld, formula %ld", w.T, l.total, formula);
    const int sections = SEC_RING | (w.with_state ? SEC_LSTM | SEC_CARRY : 0) | (w.rs_rec ? SEC_HISTORY : 0) | (w.with_cache ? SEC_CACHE : 0);
    CHECK(l.sections() == sections, "T = %d: sections 0x%x, expected 0x%x", w.T, l.sections(), sections);
  }
  CHECK(sizeof kLayouts / sizeof kLayouts[0] == 3 * 2 * 4 * 2, "%zu layouts", sizeof kLayouts / sizeof kLayouts[0]);
  CHECK(SH_MAGIC == 0 && SH_CTX_FRAMES == 1 && SH_FRAME_HZ == 2 && SH_BITS == 3 && SH_N_FRAMES == 4 && SH_MODE == 5 && SH_INPUT_HZ == 6 &&
        SH_STARTED == 7 && SH_WORDS == 8, "the header words of include/vapx.h");
}

static size_t check_headers() {
  const int M = VAPX_STATE_MAGIC, LSTM = VAPX_STATE_HAS_LSTM, CACHE = VAPX_STATE_HAS_CACHE, SPLIT = VAPX_STATE_CACHE_SPLIT, RS = VAPX_STATE_HAS_RESAMPLE;
  // engines: {ctx_frames, frame_hz, input_hz, follower, with_cache, split}
  const StateExpect lead{50, 20, 0, false, false, false}, fol{50, 20, 0, true, false, false}, lead8k{50, 20, 8000, false, false, false},
      cache32{50, 20, 0, false, true, false}, cache_split{50, 20, 0, false, true, true};
  const struct { const char* what; StateExpect e; int32_t hd[8]; StateHeaderFault want; } cases[] = {
      {"a leader's record", lead, {M, 50, 20, LSTM, 50, 0, 0, 0}, SHF_NONE},
      {"an empty window, mode 2", lead, {M, 50, 20, LSTM, 0, 2, 0, 0}, SHF_NONE},
      {"a follower's record", fol, {M, 50, 20, 0, 7, 1, 0, 0}, SHF_NONE},
      {"an 8 kHz record", lead8k, {M, 50, 20, LSTM | RS, 7, 0, 8000, 3}, SHF_NONE},
      {"a cached record", cache32, {M, 50, 20, LSTM | CACHE, 7, 0, 0, 0}, SHF_NONE},
      {"a split cached record", cache_split, {M, 50, 20, LSTM | CACHE | SPLIT, 7, 0, 0, 0}, SHF_NONE},
      {"the split bit without a cache is nobody's business", lead, {M, 50, 20, LSTM | SPLIT, 7, 0, 0, 0}, SHF_NONE},
      // one per rule
      {"magic", lead, {M + 1, 50, 20, LSTM, 7, 0, 0, 0}, SHF_MAGIC},
      {"ctx_frames", lead, {M, 49, 20, LSTM, 7, 0, 0, 0}, SHF_CTX_FRAMES},
      {"frame_hz", lead, {M, 50, 10, LSTM, 7, 0, 0, 0}, SHF_FRAME_HZ},
      {"a follower's record to a leader", lead, {M, 50, 20, 0, 7, 0, 0, 0}, SHF_ROLE},
      {"a leader's record to a follower", fol, {M, 50, 20, LSTM, 7, 0, 0, 0}, SHF_ROLE},
      {"a history offered to a 16 kHz engine", lead, {M, 50, 20, LSTM | RS, 7, 0, 8000, 0}, SHF_INPUT_RATE},
      {"no history offered to an 8 kHz engine", lead8k, {M, 50, 20, LSTM, 7, 0, 0, 0}, SHF_INPUT_RATE},
      {"a 32 kHz history offered to an 8 kHz engine", lead8k, {M, 50, 20, LSTM | RS, 7, 0, 32000, 0}, SHF_INPUT_RATE},
      {"input_hz without the bit", lead, {M, 50, 20, LSTM, 7, 0, 8000, 0}, SHF_INPUT_RATE},
      {"a cache the flags do not name", lead, {M, 50, 20, LSTM | CACHE, 7, 0, 0, 0}, SHF_CACHE},
      {"no cache where the flags name one", cache32, {M, 50, 20, LSTM, 7, 0, 0, 0}, SHF_CACHE},
      {"a split cache to an fp32 engine", cache32, {M, 50, 20, LSTM | CACHE | SPLIT, 7, 0, 0, 0}, SHF_CACHE_PATH},
      {"an fp32 cache to a split engine", cache_split, {M, 50, 20, LSTM | CACHE, 7, 0, 0, 0}, SHF_CACHE_PATH},
      {"n_frames below 0", lead, {M, 50, 20, LSTM, -1, 0, 0, 0}, SHF_N_FRAMES},
      {"n_frames above T", lead, {M, 50, 20, LSTM, 51, 0, 0, 0}, SHF_N_FRAMES},
      // two rules broken: the earlier one is named
      {"frame_hz and n_frames", lead, {M, 50, 10, LSTM, 51, 0, 0, 0}, SHF_FRAME_HZ},
      {"role and cache", lead, {M, 50, 20, CACHE, 7, 0, 0, 0}, SHF_ROLE},
      {"input rate and cache", lead8k, {M, 50, 20, LSTM | CACHE, 7, 0, 0, 0}, SHF_INPUT_RATE},
      {"cache path and n_frames", cache32, {M, 50, 20, LSTM | CACHE | SPLIT, 99, 0, 0, 0}, SHF_CACHE_PATH},
      {"magic and everything else", fol, {0, 1, 2, LSTM | CACHE, -5, 0, 9, 0}, SHF_MAGIC},
  };
  for (const auto& c : cases) {
    const StateHeaderFault got = state_header_check(c.hd, c.e);
    CHECK(got == c.want, "%s: rule %d, expected %d", c.what, (int)got, (int)c.want);
  }
  CHECK(SHF_MAGIC < SHF_CTX_FRAMES && SHF_CTX_FRAMES < SHF_FRAME_HZ && SHF_FRAME_HZ < SHF_ROLE && SHF_ROLE < SHF_INPUT_RATE &&
        SHF_INPUT_RATE < SHF_CACHE && SHF_CACHE < SHF_CACHE_PATH && SHF_CACHE_PATH < SHF_N_FRAMES, "the enum lists the rules in their order");
  return sizeof cases / sizeof cases[0];
}

int main() {
  check_layouts();
  const size_t headers = check_headers();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok: %zu layouts, %zu headers\n", sizeof kLayouts / sizeof kLayouts[0], headers);
  return 0;
}
