// Argument blocks + launchers of the non-GEMM kernels (see vap_kernels.hip).
#pragma once
#include "common.h"
#include "state_record.h"

struct Conv0Args {
  const float* audio;   // [B][2][spc]
  const int* ids;       // [B] stream ids (device) or null = identity
  float* carry;         // [S][2][320] or null (stage API: frames carry their own context)
  float* h0;            // [B*2][P0+4][256] channels-last, 2 zero guard rows each side
  const float* w;       // [10][256]
  const float* bias;    // [256]
  const float* gamma;   // [256]
  const float* beta;    // [256]
  int* frames_seen;     // [S] or null
  int* bn;              // [B] out: rows in the window this frame
  int* bhead;           // [B] out: ring slot the new embedding goes to
  int L, spc, T;
};

struct LstmArgs {
  const float* gx;      // [M][ncpc][1024] input projection + both biases, permuted gate columns
  const int* ids;       // [M/2] or null
  float* h_state;       // [S*2][256]
  float* c_state;       // [S*2][256]
  const float* wfrag;   // W_hh, fragment-major [8 w][16 kc][8 ns][64 lane][4]
  float* out;           // [M][ncpc][256]
  const float* down_wf; // downsample weight, fragment-major [ncpc][8 w][16 kc][2 ns][64 lane][4] (null: skip)
  const float* down_b;  // [256] conv bias
  const float* down_g;  // [256] LayerNorm weight
  const float* down_beta;
  float* e;             // [M][256] embeddings (written when down_wf != null)
  const float* ln0_g;   // transformer layer-0 ln_self (for en)
  const float* ln0_b;
  float* en;            // [M][256] LayerNorm(e; ln0) or null
  int M, ncpc;
};

// vapx_prefill: the encoder over a CONTIGUOUS block of audio, frames_in_chunk frames of n streams per pass.  The passes' virtual batch is
// frame-major: entry v = j * n + k is frame j (of the chunk) of batch slot k, so a frame's rows of every per-entry buffer (h0 .. gx, e, en,
// qkv_new) are one contiguous [n * 2] block and the LSTM walks the frames by advancing its pointers.
struct Conv0PrefillArgs {
  const float* audio;   // row (k, c) = audio + (k * 2 + c) * row_stride: the chunk's new samples, frame j at + j * hop; 16-byte aligned
  long row_stride;      // floats, a multiple of 4
  const int* ids;       // [n] stream ids (device) or null = identity
  const float* carry;   // [S][2][320]: what precedes frame 0 of the chunk unless prefix_in_audio
  int prefix_in_audio;  // the 320 samples in front of every row are in the block itself (every chunk but a call's first)
  float* h0;            // [V*2][P0+4][256] as Conv0Args
  const float* w;
  const float* bias;
  const float* gamma;
  const float* beta;
  const int* frames_seen;   // [S]; with bhead (a call's first chunk): bhead[k] = frames_seen % T, the ring slot of the call's first frame
  int* bhead;           // [n] or null
  int L, n, T;
};

struct LstmPrefillArgs : LstmArgs {   // M = n * 2 rows; gx, e and en hold `frames` blocks of M rows each; `out` is not written
  int frames;
};

struct PrefillFillArgs {   // ring fill of a chunk: frame g = f0 + j of the call goes to ring slot (bhead + g) % T
  float* ring;             // [S*2][T][256]
  float* ring_qkv;         // [S*2][T][768]
  const float* e;          // [fc][n*2][256]
  const float* qkv_new;    // [fc][n*2][768]
  const int* ids;
  const int* bhead;        // [n] ring slot of the call's first frame (Conv0PrefillArgs)
  int n, T, fc, f0, frames;   // a frame with g + T < frames is skipped: a later frame of the call owns its slot
  // the waves of the call's last frame (g == frames - 1, always in the last chunk) also finish the call:
  int* frames_seen;        // [S] += frames
  float* carry;            // [S][2][320] <- the last 320 samples of each row
  const float* tail;       // row (k, c)'s last 320 samples at tail + (k * 2 + c) * row_stride; 16-byte aligned
  long row_stride;
};

struct GatherArgs {
  float* ring;          // [S*2][T][256] or null (then xin is used)
  float* ring_qkv;      // [S*2][T][768] cached layer-0 Q|K|V per ring row, or null
  const float* qkv_new; // [B*2][768] this frame's layer-0 Q|K|V (when ring_qkv)
  float* qkv;           // [B*2][T][768] chronological gather target (when ring_qkv)
  int* rot;             // [B] out (ring_append_kernel): ring slot of the oldest row
  const float* e;       // [B*2][256] this frame's embeddings
  const float* xin;     // [B*2][rows_in][256] explicit context (stage API)
  const int* ids;
  const int* bn;
  const int* bhead;
  float* x0;            // [B*2][T][256] chronological, zero beyond n
  float* xn;            // LayerNorm(x0; gamma, beta)
  const float* gamma;
  const float* beta;
  int B, T, rows_in;
};

struct AttnArgs {
  const float* q;       // row (bc*T + i), stride ldq, head h at column h*64
  const float* k;
  const float* v;       // rows of channel (bc ^ swap_kv), stride ldkv
  float* out;           // [B*2*T][256]
  const int* bn;
  int T, ldq, ldkv, swap_kv;
  const int* ring_rot;  // [B] or null.  Non-null (long-window layer 0): q/k/v are the per-stream Q|K|V RINGS (slab = slot*2+channel,
                        // logical row i in ring slot (i + ring_rot[b]) % T) instead of chronological batch buffers
  const int* ids;       // [B] stream slots (null: identity); only used with ring_rot
  int n_items;          // set by launch_attention_f16x3 (persistent kernel): B * 2 channels * 4 heads
#ifdef VAPX_TRACE
  unsigned long long* trace;   // debug build: optional [grid][32] s_memtime stamps of workgroup phases (env VAPX_ATTN_TRACE, long windows)
#endif
};

struct AttnMapArgs {    // attention_map.hip: the attention WEIGHTS of one attention launch (diagnostic path, vapx_transformer_maps)
  const float* q;       // as AttnArgs: row (bc*T + i), stride ldq, head h at column h*64 (chronological buffers only)
  const float* k;       // rows of channel (bc ^ swap_kv), stride ldkv
  const int* bn;
  int T, ldq, ldkv, swap_kv;
  float* dst;           // map of (stream b, channel c, head h) at dst + (2b + c) * dst_slab + h * dst_head, rows of dst_ld floats
  long dst_slab, dst_head;
  int dst_ld;
};

struct AttnProjArgs {   // attention_proj_f16x3.hip: long-window self-attention with the Q|K|V projection inside (split path, layers >= 1)
  const float* xn;      // [B*2*T][256] LayerNorm(ln_self_attn)(x) rows of the layer (the previous layer's FFN block wrote them)
  const float* wqkvp;   // the layer's per-head weight stream (weights.frag_pack_f16x3_qkv_heads)
  float* out;           // [B*2*T][256] heads merged
  const int* bn;        // [B] valid rows
  int T;
  int n_items;          // set by the launcher: B * 2 channels * 4 heads
};

struct LastRowArgs {
  const float* x;       // [B*2][T][256]
  const int* bn;
  float* xlast;         // [B*2][256] row n-1 of every (stream, channel)
  float* xnlast;        // LayerNorm(xlast; gamma, beta)
  const float* gamma;
  const float* beta;
  int B, T;
};

struct HeadArgs {
  const float* x;       // [B*2][T][256] stereo tower outputs (a = ch 0, b = ch 1); [B*2][256] if x_last_only
  const float* o;       // [B*2][T][256] ar_channel outputs
  const float* e;       // [B*2][256]
  const int* bn;
  const int* ids;
  int* frames_seen;     // incremented when non-null
  const float* waT;     // [256 k][256 j]
  const float* wbT;
  const float* cg;
  const float* cb;
  const float* hwT;     // [256 k][256 j]
  const float* hb;
  const float* vw;      // [256]
  const float* vb;      // [1]
  const float* aw;      // [8][256]
  const float* ab;      // [8]
  float* out;           // [B][out_stride]
  int B, T, mode, out_stride, x_last_only;
};

struct WirePackArgs {   // wire_pack_kernel: up to 4 models per launch
  const float* src[4];  // [n][src_stride] output rows of model m
  float* dst;           // model-major wire block
  long dst_off[4];      // floats before model m's rows in dst
  int wf4[4];           // wire floats of model m / 4
  int n_models, n, src_stride;
};

// A trunk follower at 1/R of its leader's rate (vapx_attach_trunk): entry k < n_due is a stream whose frame completes this leader tick
// (compact slot k of the follower's chain), the entries after them are streams still collecting.  Keyed by stream id.
struct TrunkCollectArgs {
  const float* lstm_out;   // leader's [n][2][ncpc_l][256]
  float* acc;              // [S][2][(R-1)*ncpc_l][256] leader rows of each stream's frame in the making
  float* A;                // [n_due][2][R*ncpc_l][256] the follower's downsample operand
  const int* sid;          // [n] stream id of entry k
  const int* slot;         // [n] leader batch slot of entry k
  const int* pos;          // [n] leader hops this stream already holds in acc (not-due entries: where this hop goes)
  const int* frames_seen;  // [S] the follower's
  int* bn;                 // [n_due] out: rows in the follower's window this frame
  int* bhead;              // [n_due] out: ring slot of the new row
  int n, n_due, ncpc_l, R, T;
};
struct OutScatterArgs {    // compact follower rows -> the leader's batch order; a stream without a frame gets a zero row with status 2
  const float* src;        // [n_due][stride]
  float* dst;              // [n][stride]
  const int* slot;         // [n] as in TrunkCollectArgs
  int n, n_due, stride;
};
hipError_t launch_trunk_collect(const TrunkCollectArgs& a, hipStream_t st);
hipError_t launch_out_scatter(const OutScatterArgs& a, hipStream_t st);
// bn / bhead of a same-rate follower with a window of its own: bn[i] = min(fs + 1, T), bhead[i] = fs % T, fs = frames_seen[ids ? ids[i] : i]
hipError_t launch_window_meta(const int* ids, const int* frames_seen, int T, int* bn, int* bhead, int n, hipStream_t st);

struct StateIoArgs {    // state_io.hip: stream-state export / import, the bulk calls' records and the per-stream calls' internal one
  float* rec;           // [n][lay.total] records (device), sections where `lay` (state_record.h) puts them
  StateLayout lay;
  int sections;         // SEC_* mask: export writes and import applies the ring rows, frames_seen and the small sections named here
                        // (the header is always written); a section the layout lacks must not be named
  const int* ids;       // [n] stream slots (device) or null: slot = id0 + k
  int id0;
  float *ring, *ring_qkv, *h_state, *c_state, *carry;   // per-stream state bases (h_state / c_state / carry unused without their sections)
  int* frames_seen;
  int T, n;
  int hdr[8];           // export: the header words (StateHeaderWord) as they are written, SH_N_FRAMES and SH_STARTED filled in per stream
  float* rs_hist;       // engines with an input rate: [S][rs_rec] resampler history, the SEC_HISTORY section (null: none)
  int* rs_started;      // [S*2], travels as bits 0-1 of header word SH_STARTED; null: not read, not applied
  int rs_rec;           // floats per stream, a multiple of 4, at most 256
};

struct ResampleGeom { int orig, nnew, width, K, d, H; };   // resample.hip: in_hz / g, 16000 / g, filter half width, taps per phase, delay blocks, history
bool resample_geometry(int in_hz, ResampleGeom* g);   // false: not 8000 / 32000 / 48000
hipError_t launch_resample_whole(const ResampleGeom& g, long rows, long n_in, const float* x, float* y, hipStream_t st);

// pcm.hip: n raw samples (VAPX_PCM_S16 / _MULAW / _ALAW; src dword-aligned) -> n floats (dst 16-byte aligned): vapx_pcm_decode
hipError_t launch_pcm_decode(int format, long n, const void* src, float* dst, hipStream_t st);

hipError_t launch_state_export(const StateIoArgs& a, hipStream_t st);
hipError_t launch_state_import(const StateIoArgs& a, hipStream_t st);
// cache rebuild of an import without cache: xn[(k*2+c)*T + t] = LayerNorm(ring row (slot ids[k], c, t)); after the GEMM, rows t < window fill
// of qkv [n][2][T][768] go to the streams' cache slots
hipError_t launch_state_ln(const float* ring, const int* ids, int id0, float* xn, const float* gamma, const float* beta, int T, int n, hipStream_t st);
hipError_t launch_state_cache_scatter(const float* qkv, const int* ids, int id0, float* ring_qkv, const int* frames_seen, int T, int n, hipStream_t st);
hipError_t launch_conv0(const Conv0Args& a, int B, hipStream_t st);
hipError_t launch_lstm(const LstmArgs& a, hipStream_t st);
hipError_t launch_ring_append(const GatherArgs& a, hipStream_t st);
hipError_t launch_conv0_prefill(const Conv0PrefillArgs& a, int V, hipStream_t st);   // V = n * frames_in_chunk virtual entries
hipError_t launch_lstm_prefill(const LstmPrefillArgs& a, hipStream_t st);
hipError_t launch_prefill_fill(const PrefillFillArgs& a, hipStream_t st);
hipError_t launch_gather_ln(const GatherArgs& a, hipStream_t st);
hipError_t launch_attention(const AttnArgs& a, int B, hipStream_t st, bool force_xl);   // force_xl: attention_xl_kernel for any T (tests)
hipError_t launch_attention_f16x3(const AttnArgs& a, int B, hipStream_t st);   // split-precision variant (attention_f16x3.hip), same arguments
hipError_t launch_attention_proj_f16x3(const AttnProjArgs& a, int B, hipStream_t st);   // split path, layers >= 1: Q|K|V projected inside (attention_proj_f16x3.hip)
hipError_t launch_attention_map(const AttnMapArgs& a, int B, hipStream_t st);   // softmax(Q.K^T / 16 + ALiBi, causal) itself (attention_map.hip)
hipError_t launch_gather_last_ln(const LastRowArgs& a, hipStream_t st);
hipError_t launch_ln_rows(const float* x, float* y, const float* gamma, const float* beta, int rows, hipStream_t st);
hipError_t launch_attention_last(const AttnArgs& a, int B, hipStream_t st);
hipError_t launch_head(const HeadArgs& a, hipStream_t st);
hipError_t launch_wire_pack(const WirePackArgs& a, hipStream_t st);
