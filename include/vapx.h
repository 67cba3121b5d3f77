/*
 * vapx.h — C ABI of libvapx.so: MI355X-native many-stream engine for the Realtime-VAP
 * streaming forward pass (CPC encoder -> LSTM -> downsample -> per-stream context ring ->
 * 1 self + 3 self/cross GPT layers -> VAP head -> p_now / p_future / VAD).
 *
 * The reference (inokoj/VAP-Realtime) has NO FFI / plugin interface for this path: it is plain
 * Python attribute calls.  Each entry point below therefore cites the reference
 * Python call it stands in for; the ctypes binding a maintainer would add on the reference side is
 * shown in INTEGRATION.md and implemented in vap-realtime_amd/engine.py.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (hipStream_t travels as void*).
 *   - every function returns 0 on success or a negative VAPX_E_* code; no exceptions cross the
 *     ABI; vapx_last_error() returns a human-readable message for the last failure on a handle
 *     (or for a failed vapx_create when called with NULL).
 *   - ownership: the caller owns audio / output / blob memory (the blob is copied at create);
 *     the library owns device weights, per-stream state and scratch.
 *   - threading: calls on one handle must be serialised by the caller (the reference runs
 *     inference on a single thread, rvap/vap_main/vap_main.py:520-521).  Work is ordered on the
 *     HIP stream passed in; device outputs are valid after that stream is synchronised, host
 *     outputs are valid on return.
 *   - one handle per GPU; streams (dialogues) are independent, so multi-GPU = one handle per
 *     device with the stream ids partitioned by the caller (no collective).
 */
#ifndef VAPX_H_
#define VAPX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAPX_ABI_VERSION 2

/* error codes */
#define VAPX_OK 0
#define VAPX_E_INVAL (-1)    /* bad argument */
#define VAPX_E_HIP (-2)      /* HIP runtime error (see vapx_last_error) */
#define VAPX_E_NOMEM (-3)
#define VAPX_E_RANGE (-4)    /* stream id / batch size out of range */
#define VAPX_E_NODEVICE (-5) /* no gfx950 device visible */
#define VAPX_E_NUMERIC (-6)  /* host-output vapx_step only: at least one stream produced non-finite p_now / p_future / VAD / aux
                                probabilities (a poisoned LSTM / ring state, Inf audio, or |activation| >= 65504 on the
                                split-precision path).  PER STREAM, not per call: the out block is complete, every other row is
                                valid, the offending rows carry VAPX_OUT_STATUS = 1 and vapx_bad_slots() lists them; reset those
                                streams and keep serving the rest.  A NaN / Inf audio SAMPLE triggers it exactly as it poisons the
                                reference: ChannelNorm and torch.relu propagate it (encoder_components.py:64-66,103), the LSTM state
                                keeps it for good (tests/golden/poison20.npz records the unmodified reference doing so). */

/* model variants: which heads are evaluated (vap_main.py:290-307, vap_bc_main.py:272-277,
 * vap_nod_main.py:273-279) */
#define VAPX_MODE_VAP 0
#define VAPX_MODE_BC 1
#define VAPX_MODE_NOD 2

/* memory-space flags for vapx_step */
#define VAPX_AUDIO_HOST 0
#define VAPX_AUDIO_DEVICE 1
#define VAPX_OUT_HOST 0
#define VAPX_OUT_DEVICE 2
#define VAPX_IDS_DEVICE 4 /* stream_ids points to device memory (default: host) */
#define VAPX_DEFER_JOIN 8 /* with overlap groups > 1: do not make hip_stream wait for the groups at the end of the step; the
                             caller orders consumers of `out` with vapx_join.  Lets group g's next tick start while other
                             groups still finish this one.  Honoured only when the whole step is device-resident
                             (VAPX_AUDIO_DEVICE | VAPX_OUT_DEVICE, ids NULL or VAPX_IDS_DEVICE) — otherwise ignored; a step
                             whose n (or group split) differs from the previous one, or that has resets pending, first
                             joins the previous tick's groups itself. */

/* vapx_config.flags */
#define VAPX_FLAG_GROUPS_MASK 0xF     /* bits 0-3: intra-tick overlap groups (0 = default 1 = none, max 8) */
#define VAPX_FLAG_MATERIALIZE_X0 64   /* copy the context window chronologically each tick ("x0" peekable); default: layer 0 reads
                                         the embedding / Q|K|V rings in place (short and long windows alike) */
#define VAPX_FLAG_SPLIT_F16 512        /* opt-in: every contraction with bounded or scalable operands — the fused flat-row blocks (FFN,
                                         projections), the attention blocks' projections, the conv / LSTM-input GEMMs, and for windows longer
                                         than 64 frames the attention itself (Q.K^T and P.V) — as fp32-accurate 3-term split products on the
                                         f16 matrix cores (x s = hi + lo; hi.hi + lo.hi + hi.lo, fp32 accumulate, power-of-two operand scales
                                         s from row / tile maxima or static weight bounds: no input can overflow f16); same 1e-4 parity bar,
                                         same error against float64 as the default fp32-MFMA path.  vapx_create refuses the flag
                                         (VAPX_E_INVAL) for a checkpoint whose transformer weights break the static bounds (|w| >= 255) */
#define VAPX_FLAG_UNFUSED_PROJ 1024    /* long windows (T > 64): attention output projections (+ residual + LN, + cross-attention query
                                         projection) as separate GEMM launches instead of riding in the fused blocks; kept for A/B tests */
#define VAPX_FLAG_SPLIT_QKV_IN_FFN 2048 /* with VAPX_FLAG_SPLIT_F16 and windows longer than 64 frames: the self-attention Q|K|V of layers 1-2 come from the
                                         previous layer's flat-row block through HBM (rounds 2-4) instead of being projected inside the attention
                                         kernel (csrc/attention_proj_f16x3.hip); kept for A/B tests */
#define VAPX_FLAG_UNFUSED_LAST_ROW 256 /* last layer's newest-row path as ten launches (gathers, M = 2B GEMMs, single-query
                                         attention) instead of the fused last_block_kernel; kept for A/B parity tests */
#define VAPX_FLAG_UNFUSED_CONV 32     /* conv2-4 as three GEMM launches (materialises "h2","h3" for vapx_peek) */
#define VAPX_FLAG_FULL_LAST_LAYER 16  /* compute every row of the last layer (default: only the newest row,
                                         which is all process_vap consumes; needed to vapx_peek "stereo2") */

/* Layout of one output row (floats).  Row stride is VAPX_OUT_STRIDE. */
#define VAPX_OUT_P_NOW 0     /* [2]  result_p_now        vap_main.py:316 */
#define VAPX_OUT_P_FUTURE 2  /* [2]  result_p_future     vap_main.py:317 */
#define VAPX_OUT_VAD 4       /* [2]  result_vad          vap_main.py:313-320 */
#define VAPX_OUT_AUX 6       /* [4]  bc: {-, p_bc_react, p_bc_emo, -}; nod: {-, short, long, long_p} */
#define VAPX_OUT_NVALID 10   /* [1]  n = rows in the context window this frame (as float) */
#define VAPX_OUT_VAD_LOGIT 11 /* [2] va_classifier outputs before the sigmoid (what the training-style forward() returns) */
#define VAPX_OUT_STATUS 13   /* [1]  0 = ok, 1 = this row's probabilities are not finite (see VAPX_E_NUMERIC); written on device,
                                      so the device-output path carries it too; 2 = VAPX_STATUS_NO_FRAME */
#define VAPX_STATUS_NO_FRAME 2 /* a trunk follower slower than its leader (vapx_attach_trunk) had no frame due for this stream on this
                                      leader tick: the rest of the row is zero.  No fault: vapx_bad_slots, VAPX_E_NUMERIC and
                                      vapx_group_bad count status 1 only */
#define VAPX_OUT_LOGITS 16   /* [256] vap_head logits of the newest row  vap_main.py:290;
                                      nod mode: p_bc of rows 0..n-1 instead (vap_nod_main.py:276 quirk), 0 in slots n..ctx_frames-1;
                                      one slot per window row, so vapx_create refuses nod mode with ctx_frames > 256 */
#define VAPX_OUT_E 272       /* [2*256] this frame's embeddings e1,e2   vap_main.py:272 */
#define VAPX_OUT_STRIDE 784

typedef struct vapx_engine* vapx_handle;

typedef struct vapx_config {
  int32_t struct_size;  /* sizeof(vapx_config), for ABI evolution */
  int32_t device_id;    /* HIP device ordinal */
  int32_t frame_hz;     /* 5, 10, 20 or 50: VAPRealTime frame_rate   vap_main.py:192,219 */
  int32_t ctx_frames;   /* T = int(context_len_sec*frame_rate)        vap_main.py:221.  1 <= T <= 512 (vapx_create returns VAPX_E_INVAL beyond;
                         * nod mode: T <= 256, the p_bc slots of an output row).
                         * Every published checkpoint fits in 256 (largest: 20 Hz x 10 s = 200 rows, README.md; BASELINE configs[2]: 50 Hz x 5 s = 250)
                         * and that is what the long-window attention kernels are tuned for; the reference's ALiBi transformer itself takes any T
                         * (modules.py:303-308), so windows of 257 .. 512 rows run too — through a plain fp32 attention kernel (K / V from L2, no
                         * on-chip tile; on the split-precision path as well) that is correct, tested against the oracle, and not tuned */
  int32_t max_streams;  /* stream slots whose state lives in HBM */
  int32_t max_batch;    /* max streams per vapx_step call (sizes scratch) */
  int32_t mode;         /* VAPX_MODE_* */
  int32_t flags;        /* VAPX_FLAG_* */
} vapx_config;

/* Number of floats the weight blob must have for a frame rate (layout:
 * vap-realtime_amd/weights.py:blob_layout).  Returns 0 for an unsupported rate. */
size_t vapx_blob_floats(int32_t frame_hz);

/* Stands in for VAPRealTime.__init__ (vap_main.py:192-247): builds device weights from the packed
 * blob (host memory, fp32), allocates per-stream state (context ring, LSTM h/c, 320-sample
 * carry) zero-initialised, and scratch for max_batch streams. */
int vapx_create(const vapx_config* cfg, const float* weights_blob, size_t n_floats, vapx_handle* out);

void vapx_destroy(vapx_handle h);

/* Stands in for VAPRealTime.process_vap (vap_main.py:249-335) for n streams at once.
 *   stream_ids : n ids in [0,max_streams), all distinct (host ids are checked: VAPX_E_RANGE / VAPX_E_INVAL for a duplicate;
 *                device ids are the caller's responsibility); NULL means 0..n-1.
 *   audio      : fp32 [n][2][samples_per_ch].  samples_per_ch == hop (=16000/frame_hz): new
 *                samples only, the engine prepends its own 320-sample carry like proc_serv_in
 *                (vap_main.py:397-409).  samples_per_ch == hop+320: a complete frame exactly as
 *                process_vap receives x1/x2 (carry supplied by the caller, vap_offline.py:51-61);
 *                the engine's carry is then set to the frame's last 320 samples.
 *   out        : fp32 [n][VAPX_OUT_STRIDE].
 *   flags      : VAPX_AUDIO_* | VAPX_OUT_* | VAPX_IDS_DEVICE | VAPX_DEFER_JOIN
 *   hip_stream : hipStream_t to order the work on (NULL = default stream).
 * Host audio / out in vapx_host_alloc memory is copied with true async DMA; pageable memory is staged through the engine's
 * own pinned buffers (one extra memcpy each way). */
int vapx_step(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* audio,
              int32_t samples_per_ch, float* out, int32_t flags, void* hip_stream);

/* Input rate: audio at 8, 32 or 48 kHz, resampled to the model's 16 kHz on the device (csrc/resample.hip).  Telephone audio is 8 kHz
 * and WebRTC delivers 48 kHz; the published multilingual checkpoints met their 8 kHz corpora through torchaudio's default resampler
 * (train/audio.py:65-68), which is the filter used here: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99, fp32 taps
 * (vap-realtime_amd/resample.py restates it and writes the tables).  With g = gcd(input_hz, 16000), orig = input_hz / g, new = 16000 / g:
 *   Y[new*i + p] = sum_k h[p][k] * x[orig*i + k - width]   (x = 0 outside the signal), one fmaf chain over k = 0 .. K-1
 *   8000: orig 1, new 2, width 7, K 15     32000: 2, 1, 13, 28     48000: 3, 1, 19, 41
 *
 * vapx_set_input_rate: allowed once, on a freshly created engine with no step yet (the rule of vapx_attach_trunk); refused on a trunk
 * follower (the leader owns the audio) and for any rate but 8000, 16000, 32000, 48000 (VAPX_E_INVAL).  16000 is accepted and changes
 * nothing: such an engine behaves bit for bit as one that never made the call.  Otherwise the engine allocates a zeroed per-stream
 * history and from then on
 *   - vapx_step / vapx_step_group take samples_per_ch == hop_in = input_hz / frame_hz and nothing else: a full frame with the caller's
 *     carry (hop + 320) is defined at 16 kHz only; vapx_encode_audio, whose frames carry their own carry, is refused;
 *   - DELAY: a dialogue has no future samples, so the 16 kHz stream the model sees is Y delayed by d = ceil(width / orig) = 7 blocks:
 *     z[m] = Y[m - new*d], zero for m < new*d — 0.875 ms at 8 kHz, 0.4375 ms at 32 and 48 kHz.  Tick t consumes x[t*hop_in, (t+1)*hop_in)
 *     and emits z[t*hop, (t+1)*hop); the engine keeps the last H = orig*d + width input samples per stream and channel (14, 27, 40).  One
 *     launch per step, before the overlap groups fork; conv0, the 320-sample carry and everything after them see plain 16 kHz hops;
 *   - vapx_reset_stream and vapx_reset_carry zero the stream's history together with the carry: a new connection is a new signal;
 *   - VAPX_DEFER_JOIN is not honoured (the resampled hops of a tick live in one buffer).
 * vapx_get_input_rate: the rate in Hz (16000 unless another was set); on a follower 16000.
 * vapx_resample: the whole-signal Y for `rows` independent signals, device pointers, x [rows][n_in] -> y [rows][ceil(new*n_in/orig)];
 * stateless and without a handle, like vapx_softmax256; the same device function as the engine's kernel, so a stream stepped at
 * input_hz equals, bit for bit, a 16 kHz engine fed z.  16000 copies. */
int vapx_set_input_rate(vapx_handle h, int32_t input_hz);
int32_t vapx_get_input_rate(vapx_handle h);
int vapx_resample(int32_t input_hz, int64_t rows, int64_t n_in, const float* x, float* y, void* hip_stream);

/* Input format: audio in the sample format a telephone gateway or a WebRTC stack already has, decoded to the model's fp32 on the device
 * (csrc/pcm.hip).  vap-realtime_amd/pcm.py is the definition and writes the G.711 tables of csrc/pcm_tables.h:
 *   VAPX_PCM_F32    4 bytes / sample   the float itself (the default: an engine that never makes the call)
 *   VAPX_PCM_S16    2, little-endian   (float)v * 2^-15
 *   VAPX_PCM_MULAW  1                  (float)U[c] * 2^-15      U, A: the ITU-T G.711 expansions to 16-bit linear
 *   VAPX_PCM_ALAW   1                  (float)A[c] * 2^-15      (U[0x00] = -32124, U[0x7F] = U[0xFF] = 0; A[0xD5] = 8, A[0xAA] = 32256)
 * Every value is exact in fp32 and both mu-law zero codes give +0.0f: nothing rounds, so an engine stepped in a raw format equals, bit
 * for bit, an engine fed the decoded floats.
 *
 * vapx_set_input_format: the rules of vapx_set_input_rate — allowed once, on a freshly created engine with no step yet; refused on a
 * trunk follower and for an unknown id (VAPX_E_INVAL).  VAPX_PCM_F32 is accepted and changes nothing.  Independent of
 * vapx_set_input_rate: the two may be called in either order.  From then on
 *   - `audio` of vapx_step / vapx_step_group points to [n][2][samples_per_ch] SAMPLES OF THAT FORMAT: the parameter keeps its type
 *     `const float*` and is reinterpreted.  samples_per_ch keeps its meaning and its checks (hop or hop + 320 at 16 kHz, hop_in with an
 *     input rate); every legal value is a multiple of 16, so rows stay dword-aligned.  The block's base address must be 4-byte aligned
 *     (VAPX_E_INVAL otherwise).  VAPX_AUDIO_HOST (page-locked or pageable, staged as before but in bytes) and VAPX_AUDIO_DEVICE both work;
 *   - the engine's one input launch per step (csrc/input_classes.hip, the launch of an input rate) decodes the whole batch, and with an
 *     input rate resamples it in the same pass: there is no decoded intermediate.  Its output, 16 kHz fp32 rows in an engine buffer
 *     ([max_batch][2][hop + 320] at 16 kHz, [max_batch][2][hop] with an input rate), is what conv0 reads, before the overlap groups fork;
 *   - vapx_encode_audio always takes fp32 frames and is unaffected; state records, snapshots and vapx_reset_* are untouched (the decoder
 *     has no state: a record moves freely between engines of different input formats);
 *   - VAPX_DEFER_JOIN is not honoured (the decoded hops of a tick live in one buffer).
 * vapx_get_input_format: the id (VAPX_PCM_F32 unless another was set); on a follower VAPX_PCM_F32.
 * vapx_pcm_decode: n samples of `format` (S16 / MULAW / ALAW) at src -> n floats at dst, device pointers, src 4-byte and dst 16-byte
 * aligned; stateless and without a handle, like vapx_resample; the same kernel as the engine's step. */
#define VAPX_PCM_F32 0
#define VAPX_PCM_S16 1
#define VAPX_PCM_MULAW 2
#define VAPX_PCM_ALAW 3
int vapx_set_input_format(vapx_handle h, int32_t format);
int32_t vapx_get_input_format(vapx_handle h);
int vapx_pcm_decode(int32_t format, int64_t n, const void* src, float* dst, void* hip_stream);

/* Input classes: streams of DIFFERENT sample formats and rates in one engine (csrc/input_classes.hip).  vapx_set_input_rate and
 * vapx_set_input_format hold for every stream of an engine; a service that faces telephone gateways (8 kHz mu-law), WebRTC peers (48 kHz
 * s16) and clients with the reference's f64 framing at once would need one engine - weights, state, scratch, ports - per combination.  An
 * input class is a pair (sample format, sample rate); an engine gets a table of classes once, every stream belongs to one class, and ONE
 * kernel launch per step decodes and resamples the whole ragged batch.  It is the launch of vapx_set_input_rate / _format too: inside
 * the engine those are a table of one class without slot descriptors, with their own rules for the step (above).  An engine with neither
 * a rate, a format nor a table launches no input kernel.
 *
 * vapx_set_input_classes: the rules of vapx_set_input_rate - allowed once, on a freshly created engine with no step yet; refused
 * (VAPX_E_INVAL, with a message) on a trunk follower, together with vapx_set_input_rate / vapx_set_input_format in either order, for n
 * outside 1 .. VAPX_MAX_INPUT_CLASSES, for an unknown rate or format and for two equal entries.  The engine allocates the per-stream
 * history for the largest H among the classes, the `started` flags, the 16 kHz hops [max_batch][2][hop] and staging for the largest slot.
 * Every stream starts in class 0.  vapx_get_input_classes: the table (at most max entries) and its length; 0 = no table.
 *
 * vapx_set_stream_class: queued like vapx_reset_carry and applied by the next step before it touches any state: the stream's 320-sample
 * carry, its resampler history and its `started` flags are zeroed (a new class is a new signal); the LSTM and the context ring stay, as on
 * the reference's reconnect.  VAPX_E_RANGE for a bad stream id or class; VAPX_E_INVAL on an engine without a table.
 * vapx_get_stream_class: the stream's class (negative error code on a bad id or an engine without a table).
 * vapx_input_slot_bytes: bytes of one batch slot of class cls: 2 * hop_in(cls) * bytes_per_sample(cls), hop_in(c) = input_hz(c) / frame_hz;
 * 0 for a bad class or an engine without a table.
 *
 * LAYOUT of a step on an engine with a table (vapx_step and vapx_step_group): `audio` points to a PACKED block.  Slot k (batch order) holds
 * [2][hop_in(c_k)] samples of format(c_k) at byte offset sum_{j<k} vapx_input_slot_bytes(c_j), c_k = the class of stream_ids[k].  Every slot
 * size is a multiple of 16 bytes (every legal hop_in is a multiple of 16 samples); the base address must be 16-byte aligned
 * (VAPX_E_INVAL).  samples_per_ch must be 0: the classes define the sizes, and a full frame with the caller's carry is refused as with an
 * input rate.  The engine computes the offsets from the ids, so they must be on the host: VAPX_IDS_DEVICE is VAPX_E_INVAL (the rule a
 * slower trunk follower already has).  VAPX_AUDIO_HOST (page-locked or pageable, staged in bytes) and VAPX_AUDIO_DEVICE both work;
 * VAPX_DEFER_JOIN is not honoured (the hops of a tick live in one buffer).  Followers of such a leader work unchanged: the leader owns the
 * audio.  A class (f, r) stream equals, bit for bit, the stream of an engine with vapx_set_input_format(f) and vapx_set_input_rate(r): one
 * kernel, one definition of each expansion and of the resampler's chain (csrc/input_decode.h), shared with vapx_pcm_decode and vapx_resample.
 *
 * Other calls: vapx_encode_audio is refused, as with an input rate.  vapx_get_state / vapx_set_state behave as with an input rate (the
 * history restarts).  DELIBERATE GAPS: vapx_export_streams / vapx_import_streams are REFUSED (VAPX_E_INVAL) - a state record has one history
 * size per engine, records with per-stream history sizes are a follow-up (the precedent of the mixed-rate follower); the group and door front-ends
 * (vapx_ingest_open_group*, passive shards behind vapx_frontdoor_*) refuse a table - vapx_ingest_open and vapx_ingest_open_fn serve one, with an
 * input port per class (vapx_ingest_config.input_classes); offline.py keeps
 * its one engine per rate (its 16 kHz pairs use full frames with a real carry, which a class engine refuses by design).
 *
 * CHANNEL CLASSES: a class belongs to a (stream, channel).  A contact-centre dialogue has an agent leg from a softphone (48 kHz s16) and a
 * customer leg from the PSTN (8 kHz G.711); a gateway that forks both legs has them in two codecs.  vapx_set_stream_class(sid, c) means
 * (c, c), and everything above holds for such a stream as it stands.
 * vapx_set_stream_channel_classes(sid, c1, c2): the rules of vapx_set_stream_class - queued, applied by the next step before it touches any
 * state; the carry, the history and the `started` flags of BOTH channels are zeroed, the LSTM and the ring stay.  VAPX_E_RANGE for a bad
 * stream id or class; VAPX_E_INVAL on an engine without a table.  A reset of one channel alone, where only one leg's class changes, is
 * deliberately not built: the 320-sample carry and the reset list are per stream, and a leg that changes codec in mid-call is a new call.
 * vapx_get_stream_channel_classes: out[0], out[1] = the classes of channel 1 and channel 2.  vapx_get_stream_class returns c where both
 * are c and VAPX_E_INVAL (with a message naming this call) where they differ.
 * vapx_input_row_bytes: bytes of ONE channel's row of class cls, hop_in(cls) * bytes_per_sample(cls), a multiple of 16; 0 for a bad class
 * or an engine without a table.  vapx_input_slot_bytes(c) = 2 * vapx_input_row_bytes(c), unchanged.
 * LAYOUT: slot k of the packed block holds channel 1's row, hop_in(c1) samples of format(c1), followed by channel 2's row, hop_in(c2)
 * samples of format(c2): vapx_input_row_bytes(c1) + vapx_input_row_bytes(c2) bytes, at the sum of the earlier slots' sizes.  For c1 == c2
 * this is the layout above byte for byte; every row is a multiple of 16 bytes, so every alignment rule stays.  A mixed slot is never
 * larger than the largest same-class slot of the table, so the staging, the LDS window and the 4 GiB rule of vapx_set_input_classes
 * stand.  Each channel's history lives in its own half of the stream's record, whatever the other channel's class.
 * SKEW: each channel reaches the model with its own class's delay (DELAY under "Input rate"), d = 7 blocks of `new` 16 kHz samples: 0.875 ms
 * at 8 kHz, 0.4375 ms at 32 and at 48 kHz, none at 16 kHz.  Two legs of different classes are therefore up to 0.875 ms apart, against a frame
 * of 20 - 100 ms. */
#define VAPX_MAX_INPUT_CLASSES 16      /* 4 formats x 4 rates: every combination fits */
typedef struct vapx_input_class { int32_t input_hz; int32_t format; } vapx_input_class;   /* 8000|16000|32000|48000, VAPX_PCM_* */
int vapx_set_input_classes(vapx_handle h, int32_t n, const vapx_input_class* classes);
int32_t vapx_get_input_classes(vapx_handle h, vapx_input_class* out, int32_t max);
int vapx_set_stream_class(vapx_handle h, int32_t stream_id, int32_t cls);
int32_t vapx_get_stream_class(vapx_handle h, int32_t stream_id);
int64_t vapx_input_slot_bytes(vapx_handle h, int32_t cls);
int vapx_set_stream_channel_classes(vapx_handle h, int32_t stream_id, int32_t cls_ch1, int32_t cls_ch2);
int vapx_get_stream_channel_classes(vapx_handle h, int32_t stream_id, int32_t out[2]);
int64_t vapx_input_row_bytes(vapx_handle h, int32_t cls);

/* Batch slots (row indices of `out`) of the latest host-output vapx_step whose results were not finite; returns their number
 * (writes at most max_slots of them; slots may be NULL to just count). */
int32_t vapx_bad_slots(vapx_handle h, int32_t* slots, int32_t max_slots);

/* Page-locked host memory for audio / out blocks (hipHostMalloc): vapx_step then DMAs straight from / into it.
 * NULL on failure.  Not tied to a handle. */
void* vapx_host_alloc(size_t bytes);
void vapx_host_free(void* p);

/* Make hip_stream wait for every overlap group of the latest vapx_step (see VAPX_DEFER_JOIN). */
int vapx_join(vapx_handle h, void* hip_stream);

/* Multi-model serving on one shared CPC trunk.  The bc / nod / vap programs of the reference
 * (rvap/vap_bc/vap_bc_main.py, rvap/vap_nod/vap_nod_main.py, rvap/vap_main/vap_main.py) each load the SAME cpc_model
 * file for the CNN + LSTM (vap_main.py:199-201 skips the state dict's encoder.* keys) and differ only in the
 * downsample, the transformer and the heads.  After vapx_attach_trunk(follower, leader) the follower never runs the
 * encoder: each tick, step the leader with the audio, then step every follower with audio == NULL (same n, same
 * hip_stream; stream_ids is ignored, the leader's are used).  The follower applies its own downsample to the
 * leader's LSTM outputs and runs its own rings / transformer / heads.  Requirements: both engines freshly created
 * (no step yet), same device, max_streams, max_batch, and bit-identical CPC weights in the two blobs.  A leader can
 * have several followers; vapx_reset_stream on the leader resets them too (and is refused on a follower); LSTM /
 * carry state import / export goes through the leader, ring state through each engine.  Destroy followers before
 * their leader.
 *
 * Mixed groups (the reference deploys vap at 20 Hz / 2.5 s next to bc at 20 Hz / 5 s and nod at 10 Hz / 10 s, README.md).
 * ctx_frames may differ from the leader's: the follower then fills and slides its own window (a follower with the leader's rate
 * and window runs exactly the path it ran before, bit for bit).  frame_hz may differ when the leader's rate is an integer
 * multiple R of the follower's (50 -> 10, 50 -> 5, 20 -> 10, 20 -> 5, 10 -> 5; 50 -> 20 and a leader slower than its follower are
 * refused): the group's fastest model leads.  A CPC frame is a function of real samples only and the LSTM carries (h, c) from frame
 * to frame, so the R * n_cpc LSTM rows of a follower's frame are those of R consecutive leader ticks.  Such a follower
 *   - is still stepped every leader tick, with the leader's n.  Per stream it collects the leader's rows (trunk_collect_kernel, keyed
 *     by stream id: batches may be ragged and reorder) and runs its own chain on every R-th tick OF THAT STREAM, counted from the
 *     stream's reset.  out[n][VAPX_OUT_STRIDE] keeps the leader's batch order; a row without a frame is all zero with
 *     VAPX_OUT_STATUS = VAPX_STATUS_NO_FRAME.  In vapx_step_group the wire row being a prefix of the output row, a slower model's
 *     wire rows carry status 2 on ticks without a frame.
 *   - needs the leader's stream ids on the host: after a leader step with VAPX_IDS_DEVICE its step returns VAPX_E_INVAL.
 *   - does not honour VAPX_DEFER_JOIN (it joins its overlap groups, which split the due streams, before it returns).
 *   - vapx_reset_stream on the leader restarts the stream's frame as well; vapx_reset_carry leaves it alone, as the reference's
 *     reconnect leaves its model state.
 *   - vapx_get_state / vapx_set_state move its ring as on any follower; vapx_export_streams / vapx_import_streams are REFUSED
 *     (VAPX_E_INVAL): a state record does not carry the half-collected frame and the phase yet.  Same-rate followers with a window
 *     of their own export and import as before (their records carry ctx_frames). */
int vapx_attach_trunk(vapx_handle follower, vapx_handle leader);

/* The whole trunk group in ONE call, answered with compact wire rows (multi-model serving: vap_main.py, vap_bc_main.py and
 * vap_nod_main.py side by side on one cpc_model file).
 *
 * The wire row of a model is the head of its vapx_step output row — exactly what its result packet is built from (util.py:122-143 vap,
 * :193-211 bc, :213-237 nod):
 *   floats [0, 16)   p_now, p_future, vad, aux, n-valid, vad logits, status (VAPX_OUT_P_NOW .. VAPX_OUT_STATUS and two reserved floats)
 *   nod only         the next T floats (VAPX_OUT_LOGITS + 0 .. T-1): p_bc of every window row (the quirk of vap_nod_main.py:276)
 * vapx_wire_floats(mode, ctx_frames) is its length: 16 for vap and bc, 16 + T rounded up to a multiple of 4 for nod (rows stay 16-byte
 * aligned; the padding floats are the output row's next floats); 0 for a bad mode / window.  A wire row being a prefix of an output
 * row, vapx_wire_encode_result takes it unchanged.  vapx_group_wire_floats(leader) is the sum over the leader and its followers, per
 * stream (0 for a follower).
 *
 * vapx_step_group(leader, ...) steps the leader, then every follower in attach order — all device-resident on hip_stream, the path
 * vapx_step takes with VAPX_OUT_DEVICE — and gathers the wire rows with one kernel into one block, model-major:
 *   wire_out [model m][n][wire_floats(m)], model m's rows starting at float n * (wire_floats(0) + .. + wire_floats(m-1));
 *   model 0 is the leader, model i + 1 the i-th attached follower.
 * stream_ids / audio / samples_per_ch as in vapx_step; flags: VAPX_AUDIO_* | VAPX_IDS_DEVICE | VAPX_OUT_*.  With VAPX_OUT_HOST the tick
 * costs ONE linear device-to-host copy and ONE synchronisation (M host-output vapx_step calls copy M x n x 784 floats and synchronise M
 * times; a bc packet needs 2 of those floats); vapx_host_alloc memory is written directly, pageable memory is staged.  With
 * VAPX_OUT_DEVICE wire_out is device memory: no copy, no synchronisation.  VAPX_DEFER_JOIN is NOT honoured: the gather consumes every
 * overlap group's rows.
 * VAPX_E_NUMERIC (host output only) is per stream and per model as in vapx_step: the block is complete, the offending rows carry
 * VAPX_OUT_STATUS = 1 in every model that produced non-finite values, and vapx_group_bad lists the (batch slot, model index) pairs
 * (returns their number, writes at most max; either array may be NULL).  Reset such a stream on the leader.
 * Refused with VAPX_E_INVAL: on a follower, and on a leader whose followers have not all consumed its latest plain vapx_step.
 * vapx_peek, vapx_get_state / vapx_set_state and vapx_reset_stream behave after it as after the separate calls. */
int32_t vapx_wire_floats(int32_t mode, int32_t ctx_frames);
size_t vapx_group_wire_floats(vapx_handle leader);
int vapx_step_group(vapx_handle leader, int32_t n, const int32_t* stream_ids, const float* audio, int32_t samples_per_ch,
                    float* wire_out, int32_t flags, void* hip_stream);
int32_t vapx_group_bad(vapx_handle leader, int32_t* slots, int32_t* models, int32_t max);

/* Zero one stream's state (context ring fill, LSTM h/c, carry; with an input rate the resampler history too).  The reference never resets
 * model state on reconnect (vap_main.py:368-369 re-zeroes only the carry); this is the explicit
 * equivalent of constructing a fresh VAPRealTime for that stream.
 * Stream-ordered and free for everybody else: the call only queues the request (no device work, no synchronisation); the
 * next vapx_step / vapx_encode_audio applies it on its HIP stream before touching any state, and vapx_get_state /
 * vapx_set_state / vapx_peek apply it before they look. */
int vapx_reset_stream(vapx_handle h, int32_t stream_id);

/* Zero only the 320-sample carry of a stream (and, with an input rate, its resampler history): exactly what the reference does when an input client (re)connects
 * (vap_main.py:368-369: current_x1 / current_x2 restart from zeros, LSTM and context are kept).  Queued and stream-ordered
 * like vapx_reset_stream. */
int vapx_reset_carry(vapx_handle h, int32_t stream_id);

/* The configuration a handle was created with. */
int vapx_get_config(vapx_handle h, vapx_config* out);

/* State export / import for one stream (tests, migration between GPUs).  Host pointers, any may
 * be NULL to skip.  ring: [2][T][256] oldest->newest, rows >= n_frames undefined;
 * lstm: [2 ch][2 (h,c)][256]; carry: [2][320].  The resampler history of an engine with an input rate has no place in these calls:
 * vapx_set_state ZEROES it (the stream's input continues as a new signal); vapx_export_streams / vapx_import_streams carry it.
 * They work on every engine, input classes and trunk followers at any rate included.
 *
 * Ordering: synchronising.  Argument checks first - a refused call reads and writes nothing: a vapx_get_state refused for a follower's
 * lstm / carry leaves ring and n_frames as the caller had them, and a follower whose leader was destroyed is refused the same way
 * (VAPX_E_INVAL; its LSTM / carry buffers went with the attach).  Then the device is made idle and queued resets are applied (as vapx_peek
 * does), and the call moves the stream with the bulk calls' kernels on the NULL stream - ordered against a caller's blocking streams as a
 * null-stream call is - through one copy, and returns after one synchronisation of that stream; host buffers are valid / reusable on
 * return.  vapx_set_state with a ring rebuilds the layer-0 Q|K|V cache of rows t < n_frames as an import without VAPX_STATE_CACHE does (one
 * LayerNorm, one GEMM, one scatter); cache rows t >= n_frames stay as they were: nothing reads them before the step that appends row t
 * rewrites them. */
int vapx_get_state(vapx_handle h, int32_t stream_id, float* ring, int32_t* n_frames, float* lstm, float* carry);
int vapx_set_state(vapx_handle h, int32_t stream_id, const float* ring, int32_t n_frames, const float* lstm,
                   const float* carry);

/* Bulk state export / import: snapshot, restore and migrate MANY streams in one stream-ordered call (a rolling restart, an upgrade, a
 * GPU drain: INTEGRATION.md "Snapshots and migration").  The reference keeps the LSTM (h, c) of a dialogue for good and needs 2.5 - 10 s to
 * refill its context window (vap_main.py:274-283), so a stream restarted from zeros never again matches the uninterrupted one.
 *
 * One fixed-size RECORD per stream, vapx_state_floats(h, flags) floats long (a multiple of 4: records stay 16-byte aligned), in order:
 *   header  8 x int32 (32 bytes, stored in the float slots bit for bit):
 *             [0] VAPX_STATE_MAGIC   [1] ctx_frames   [2] frame_hz
 *             [3] content bits: VAPX_STATE_HAS_LSTM (LSTM + carry follow), VAPX_STATE_HAS_CACHE (the Q|K|V cache follows the ring),
 *                 VAPX_STATE_CACHE_SPLIT (that cache was made by an engine created with VAPX_FLAG_SPLIT_F16)
 *             [4] n_frames, 0 .. T: valid ring rows   [5] the exporting engine's mode (informational)   [6], [7] zero — unless the
 *                 engine has an input rate (vapx_set_input_rate): then [3] has VAPX_STATE_HAS_RESAMPLE, [6] is input_hz and bits 0 / 1 of [7]
 *                 say that channel 1 / 2 has consumed a tick since the stream's reset (before that the first d blocks are silent)
 *   lstm    [2 ch][2 (h, c)][256] and carry [2][320] (1664 floats) - a stand-alone engine or a trunk leader only.  A trunk follower's
 *           records omit them: that state lives in its leader
 *   history only with VAPX_STATE_HAS_RESAMPLE: the resampler's input history [2][H] (H = 14, 27, 40 at 8, 32, 48 kHz), padded with zeros to a
 *           multiple of 4 floats (28, 56, 80), after the carry.  Records of engines without an input rate are byte for byte what they were
 *   ring    [2][T][256] chronological, oldest -> newest; rows t >= n_frames are written as ZEROS, so a blob is deterministic and never
 *           carries uninitialised (or VAPX_POISON_SCRATCH) memory
 *   cache   only with VAPX_STATE_CACHE: the layer-0 Q|K|V cache [2][T][768], same order, same zero fill
 * Record k of a call belongs to stream_ids[k] and starts at float k * vapx_state_floats(h, flags).
 *
 *   n          : 1 .. max_streams (NOT limited by max_batch)
 *   stream_ids : n distinct ids, host (checked as in vapx_step) or device (VAPX_IDS_DEVICE, unchecked); NULL means 0..n-1
 *   dst / src  : the records; host memory (VAPX_OUT_HOST) or device memory (VAPX_OUT_DEVICE) - the bit names the space for both calls
 *   flags      : VAPX_STATE_CACHE | VAPX_OUT_HOST / VAPX_OUT_DEVICE | VAPX_IDS_DEVICE
 *
 * Ordering: like a step.  The call makes hip_stream wait for overlap groups a VAPX_DEFER_JOIN step left running, applies queued
 * vapx_reset_stream / vapx_reset_carry requests, then enqueues its work on hip_stream.  No device-wide synchronisation anywhere.  With a
 * device buffer: no synchronisation at all, ONE gather (scatter) kernel for the whole call; work enqueued later on that stream sees the
 * records (the imported state).  With a host buffer the records travel through a bounded device
 * staging block (at most 32 MiB, or one record), one kernel and one copy per block: vapx_host_alloc memory is the DMA target / source itself
 * and the call synchronises hip_stream ONCE, at its end; pageable memory is staged block by block through a pinned buffer of the same
 * bounded size (one event wait per block) - never a second full-size pinned copy.  Host buffers are valid / reusable on return.
 *
 * Import: ring rows land in slots 0 .. n_frames-1, the window fill becomes n_frames, LSTM and carry go to the stream's slots.
 *   - with VAPX_STATE_CACHE the cache rows are scattered as they are: no LayerNorm, no GEMM is launched, and the continuation consumes
 *     exactly the cached values the source engine had - on the same checkpoint and flags it is BIT-IDENTICAL to the uninterrupted stream
 *     (tests/test_state_bulk_gpu.py asserts equality, not a tolerance).  Such records go only into an engine of the same precision path
 *     (VAPX_FLAG_SPLIT_F16 set or clear on both sides: the cached values differ); a mismatch is VAPX_E_INVAL;
 *   - without it the cache is rebuilt as vapx_set_state does, LN(ring rows) . Wqkv^T on the fp32 path, batched over the streams of the
 *     call in chunks of max_batch through the engine's scratch: three launches per chunk however many streams it holds.  Such records are
 *     portable between the two precision paths; the continuation is then close to the uninterrupted one (1e-5), not equal.
 * Validation happens on the host before anything is enqueued - a refused call modifies NO stream: n (VAPX_E_RANGE), host ids (VAPX_E_RANGE
 * out of range, VAPX_E_INVAL duplicate), and for a host src every record's header: magic, ctx_frames, frame_hz, content bits (VAPX_E_INVAL:
 * a leader / stand-alone record has VAPX_STATE_HAS_LSTM and is refused by a follower, and the reverse; VAPX_STATE_HAS_CACHE must agree
 * with the flag; VAPX_STATE_CACHE_SPLIT with the engine; VAPX_STATE_HAS_RESAMPLE and input_hz with the engine's input rate) and n_frames in [0, T] (VAPX_E_RANGE); vapx_last_error names the record index
 * and the field.  A DEVICE src cannot be read without a synchronisation: the kernel clamps n_frames into [0, T] and trusts the rest - the
 * caller vouches for records it keeps on the device (they came from vapx_export_streams of a matching engine).
 * Trunk groups: export / import on the leader moves LSTM + carry + the leader's ring, on a follower that follower's ring (+ cache);
 * after importing a stream into the leader AND every follower, vapx_step_group and the plain leader / follower steps continue as if the
 * stream had been stepped there. */
#define VAPX_STATE_CACHE 16         /* flags bit of vapx_state_floats / vapx_export_streams / vapx_import_streams */
#define VAPX_STATE_MAGIC 0x31535056 /* "VPS1" */
#define VAPX_STATE_HAS_LSTM 1
#define VAPX_STATE_HAS_CACHE 2
#define VAPX_STATE_CACHE_SPLIT 4
#define VAPX_STATE_HEADER_FLOATS 8
enum { VAPX_STATE_HAS_RESAMPLE = 8 }; /* content bit of records with a resampler history; an enumerator: the macros above are the vocabulary
                                         of records without one */
size_t vapx_state_floats(vapx_handle h, int32_t flags);
int vapx_export_streams(vapx_handle h, int32_t n, const int32_t* stream_ids, float* dst, int32_t flags, void* hip_stream);
int vapx_import_streams(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* src, int32_t flags, void* hip_stream);

/* Prefill: attach to a call in progress - fill the context window from buffered AUDIO in one call (INTEGRATION.md "Attaching to a call in
 * progress").  A stream that starts from zeros is blind for the length of its window and its LSTM never matches the uninterrupted one
 * (above); a snapshot helps only where another engine holds the state.  Where only the audio exists - a call transferred in, a recorder's
 * last seconds, a restart without a snapshot - the one way in was `frames` calls of vapx_step, each running the whole transformer for rows
 * nobody reads.  The CPC CNN is independent per frame and only h . W_hh of the LSTM is sequential; the window needs the embeddings and
 * their layer-0 Q|K|V rows and no transformer pass at all.
 *
 *   n          : 1 .. max_batch
 *   stream_ids : as in vapx_step: host ids are checked (VAPX_E_RANGE out of range, VAPX_E_INVAL for a duplicate), device ids
 *                (VAPX_IDS_DEVICE) are the caller's responsibility; NULL means 0..n-1
 *   audio      : fp32 [n][2][frames * hop], contiguous 16 kHz NEW samples (hop = 16000 / frame_hz), 16-byte aligned;
 *                host (VAPX_AUDIO_HOST, page-locked or pageable) or device (VAPX_AUDIO_DEVICE) memory
 *   frames     : >= 1, no upper bound: the work proceeds in chunks of floor(max_batch / n) frames (at least one) through the step's scratch
 *   flags      : VAPX_AUDIO_HOST | VAPX_AUDIO_DEVICE, VAPX_IDS_DEVICE
 *
 * Meaning: the state of every named stream is what `frames` consecutive calls of vapx_step(..., samples_per_ch = hop, ...) on that audio
 * would have left, except that NO output row is produced and NO transformer layer runs:
 *   - LSTM (h, c) advanced through frames * n_cpc steps; the first frame's 320-sample prefix is the stream's current carry, as in a step,
 *     and the carry becomes the block's last 320 samples;
 *   - frame j lands in ring slot (frames_seen + j) mod T; for frames > T only the last T rows are written (the LSTM still runs every
 *     frame); frames_seen += frames;
 *   - the layer-0 Q|K|V cache rows of the written slots are made as the step makes them: LN0 of the embedding (inside the LSTM kernel),
 *     then the engine's own GEMM dispatch on Wqkv - on a VAPX_FLAG_SPLIT_F16 engine the split product, like a step's;
 *   - the next vapx_step continues as if the frames had been stepped.  The arithmetic is the step's; a GEMM over another number of rows
 *     may pick another tile, so the state agrees with the stepped one to rounding, not bit for bit: tests/test_prefill_gpu.py holds small
 *     chunks (every GEMM in the 32-row tile) against float64 at twice the stepped engine's own error, tests/test_prefill_classes_gpu.py
 *     holds chunks of hundreds to 1840 entries (64- and 128-row tiles, the GEMM chain, chunks longer than the window, 50 / 20 / 10 / 5 Hz)
 *     against float64 at the encoder-stage bound.
 * Ordering: as vapx_export_streams.  The call makes hip_stream wait for overlap groups a VAPX_DEFER_JOIN step left running, applies queued
 * vapx_reset_stream / vapx_reset_carry requests, then enqueues on hip_stream; no device-wide synchronisation.  Device audio is read where it
 * lies: no copy, no synchronisation at all.  Host audio travels chunk by chunk through the step's own audio staging (one strided copy per
 * chunk from vapx_host_alloc memory; pageable memory through the pinned block, one event wait per chunk) - never a second full-size pinned
 * copy - and the call synchronises hip_stream ONCE, at its end.  Streams not named are not touched, not by a single byte.  vapx_peek after
 * a prefill names the buffers of its LAST CHUNK until the next step: "h0", "h1", "z", "e" - and "h2", "h3" unless that chunk ran the fused
 * conv tail - as [V * 2] blocks of V = n * frames_in_chunk entries, frame-major (entry v = j * n + k is frame j of the chunk and stream k of
 * the call); "lstm_out" (the prefill's LSTM launch does not write it) and every transformer buffer are refused (VAPX_E_INVAL).
 * Refused in this version (VAPX_E_INVAL, vapx_last_error names the reason; validation happens before anything is enqueued, a refused call
 * modifies nothing): an engine with an input rate, an input format or an input-class table (the resampler history would have to be
 * advanced over a long block); a trunk leader or follower (the followers' windows and collect state would have to advance too);
 * n > max_batch; frames < 1; an audio block that is not 16-byte aligned.  Ragged `frames` per stream: group equal lengths. */
int vapx_prefill(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* audio, int32_t frames, int32_t flags,
                 void* hip_stream);

/* Stage-level entry points: the model-attribute surface process_vap calls (SURVEY.md §8b level 1).
 * All pointers are DEVICE memory, fp32, contiguous.  They use the handle's weights and scratch
 * but touch no stream state except vapx_encode_audio (LSTM h/c of the given stream ids). */

/* VapGPT.encode_audio (vap_main.py:175-180): frames [n][2][hop+320] -> e [n][2][256].
 * Stateful: advances the LSTM state of stream_ids (host pointer, NULL = 0..n-1). */
int vapx_encode_audio(vapx_handle h, int32_t n, const int32_t* stream_ids, const float* frames, float* e,
                      void* hip_stream);

/* GPT.forward (ar_channel, vap_main.py:285-286) then GPTStereo.forward (ar, :287) on explicit
 * context tensors x [n][2][rows][256] (rows <= ctx_frames).  Any output pointer may be NULL.
 *   o    [n][2][rows][256]  ar_channel(x_c)["x"]
 *   x12  [n][2][rows][256]  ar(...)["x1"], ["x2"]
 *   comb [n][rows][256]     ar(...)["x"]  (Combinator output, all rows)
 *   stage 0: both; 1: ar_channel only (x -> o); 2: ar only (x is then o1,o2 -> x12, comb). */
int vapx_transformer(vapx_handle h, int32_t n, int32_t rows, const float* x, float* o, float* x12, float* comb,
                     int32_t stage, void* hip_stream);

/* vapx_transformer plus the attention weights the reference returns with attention=True (modules.py:82-110,356-423).
 * attn       [n][2][1][4][rows][rows]  ar_channel(x_c, attention=True)["attn"], channel c on dim 1
 * self_attn  [n][2][3][4][rows][rows]  ar(..., attention=True)["self_attn"]
 * cross_attn [n][2][3][4][rows][rows]  ar(..., attention=True)["cross_attn"]
 * Any pointer may be NULL; attn needs stage 0|1, self_attn / cross_attn need stage 0|2. */
int vapx_transformer_maps(vapx_handle h, int32_t n, int32_t rows, const float* x, float* o, float* x12, float* comb,
                          int32_t stage, float* attn, float* self_attn, float* cross_attn, void* hip_stream);

/* The head callables process_vap applies to tensors of any row count (vap_main.py:290-307); device pointers, rows x 256 fp32:
 *   vapx_vap_head       logits = vap_head(x)            Linear(256, 256) + bias   (vap_main.py:131,290)   [rows][256]
 *   vapx_va_classifier  y = va_classifier(x)            Linear(256, 1) + bias, BEFORE the sigmoid (:142,292-293)   [rows]
 *   vapx_aux_head       y = bc_head(x) / nod_head(x)    the bc / nod variants' extra Linear heads as vap_realtime/model.py:197,217-218
 *                       applies them to out["x"] (vap_realtime/vap_models.py:220 Linear(256, 3); :328-329 Linear(256, 4) + Linear(256, 1));
 *                       which = VAPX_AUX_BC_HEAD | VAPX_AUX_NOD_HEAD; raw outputs BEFORE softmax / sigmoid   [rows][3 | 1 | 4]
 *   vapx_softmax256     probs = logits.softmax(-1)      (:295)
 *   vapx_aggregate      objective.probs_next_speaker_aggregate(probs, from_bin, to_bin) (objective.py:186-206)   [rows][2] */
int vapx_vap_head(vapx_handle h, int64_t rows, const float* x, float* logits, void* hip_stream);
int vapx_va_classifier(vapx_handle h, int64_t rows, const float* x, float* y, void* hip_stream);
#define VAPX_AUX_BC_HEAD 0
#define VAPX_AUX_NOD_HEAD 1
int vapx_aux_head(vapx_handle h, int32_t which, int64_t rows, const float* x, float* y, void* hip_stream);
int vapx_softmax256(int64_t rows, const float* x, float* y, void* hip_stream);
int vapx_aggregate(int64_t rows, const float* probs, int32_t from_bin, int32_t to_bin, float* out, void* hip_stream);

/* Copy an internal scratch buffer of the LAST vapx_step to the host (per-layer parity tests).
 * name: "h0".."h3","z","lstm_out","e","x0","o","stereo0".."stereo2","last","comb"; returns the number of
 * floats written (<= max_floats) or a negative error.  "h2"/"h3" are refused when any overlap group of that step ran the
 * fused conv tail (VAPX_FLAG_UNFUSED_CONV always materialises them), "stereo2" needs VAPX_FLAG_FULL_LAST_LAYER, and a trunk
 * follower refuses the encoder buffers it released (peek its leader).  After a vapx_prefill and until the next step the encoder buffers are
 * those of the prefill's last chunk and everything else is refused ("Prefill" above).
 * "last": [n*2][256], the last layer's output for the newest row of every (stream, channel), where that layer runs on the newest
 * row alone (the default fused block and VAPX_FLAG_UNFUSED_LAST_ROW; one peek spans the overlap groups); with
 * VAPX_FLAG_FULL_LAST_LAYER or in nod mode it is refused: take row n - 1 of "stereo2".
 * "comb": nod mode only, [n][ctx_frames][256], the combinator of every window row (rows >= a stream's n undefined); refused in
 * the other modes and when the latest step ran in more than one overlap group (the groups' blocks are not contiguous).
 * Debug: "guard_violations" writes one float, the number of canary bytes overwritten around the process's engine allocations (-1 unless
 * the library was started with VAPX_GUARD_ZONES=1; INTEGRATION.md "Debug and experiment knobs"); "guard_selftest" changes one canary
 * byte of an allocation of its own and writes what that counter then says: 1 (-1 without the variable). */
int64_t vapx_peek(vapx_handle h, const char* name, float* dst, size_t max_floats);

/* Standalone fp32-MFMA GEMM used by every dense contraction of the path (kernel unit tests):
 * C[M][N] = epilogue(A[M][K] . W[N][K]^T); device pointers.  epi: 0 store(+bias) 1 gelu
 * 2 +resid 3 +resid & LN copy -> C2  4 bias+ChannelNorm+ReLU  5 bias+LN+GELU.  N must be a
 * multiple of 256, K a multiple of 32; epilogues 3,4,5 need N == 256. */
int vapx_gemm(void* hip_stream, int32_t M, int32_t N, int32_t K, const float* A, const float* W, float* C,
              int32_t epi, const float* bias, const float* gamma, const float* beta, const float* resid,
              float* C2, int32_t tile_rows);

/* Rows per workgroup (32, 64 or 128) that tile_rows = 0 means for a GEMM of this shape and epilogue: the engine's own dispatch rule, for
 * tests that must know which tile class a shape reaches.  Host arithmetic only: no device, no handle. */
int vapx_gemm_tile_rows(int32_t M, int32_t N, int32_t K, int32_t epi);

/* Per-kernel-class timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * class ids: 0..4 = the GEMM by epilogue (vapx_gemm's epi 0..4), 5 fused conv2-4 tail, 6 fused FFN block,
 * 7 last-row path of the final layer, 8 conv0, 9 lstm,
 * 10 ring gather+LN, 11 attention, 12 heads, 13 the GEMM with epilogue 5 (bias + LayerNorm + GELU: a trunk follower's
 * downsample, nod's Combinator on all rows), 14 the long-window mode-2 flat-row block (attention output projection + ln_src_attn + cross-attention
 * query projection; the FFN block proper stays class 6), 15 a slower trunk follower's collect and output scatter (pure copies).  enable(mask) selects classes (0 = off);
 * read() synchronises the device, sums the elapsed time and launch count per class since the
 * last read into total_ms[n_classes] / launches[n_classes], and recycles the events. */
#define VAPX_PROF_CLASSES 16
int vapx_profile_enable(vapx_handle h, uint32_t class_mask);
int vapx_profile_read(vapx_handle h, double* total_ms, int64_t* launches, int32_t n_classes);

/* ------------------------------------------------------------------------------------------------------------------
 * Native many-stream TCP front-end with the reference's packet framing.
 *
 * Stands in for proc_serv_in / proc_serv_out / proc_serv_out_dist (rvap/vap_main/vap_main.py:338-457) and the codec
 * rvap/common/util.py:52-237, for MANY dialogues in one process: the reference accepts exactly one input client
 * (`s.listen(1)`, :360-366) and decodes every sample with a Python struct.unpack.  Here: epoll receive threads decode the
 * 2560-byte packets (160 x {f64 ch1, f64 ch2}, little-endian) straight into page-locked staging (f64 -> f32 cast as
 * vap_main.py:266-270; optional gain multiplied in float64 first, :393-395), a tick thread steps every stream whose frame is
 * complete (vapx_step, host in / host out), and sender threads write the length-prefixed result packets
 * (u32 len | f64 t | u32 n | x1 | u32 n | x2 | u32 2 | p_now | u32 2 | p_future | u32 2 | vad, util.py:122-143; bc / nod variants
 * :193-237) byte-identical to the reference codec.
 *   - every connection accepted on port_in becomes a stream (lowest free slot); the 320-sample carry lives on the device
 *     and is re-zeroed for a new connection like vap_main.py:368-369 (reset_on_connect additionally clears the LSTM /
 *     context state, which the reference keeps);
 *   - every connection accepted on port_out is attached to the stream with the fewest listeners (lowest index first), i.e.
 *     the k-th output connection hears the k-th input stream; broadcast = 1 sends every result to every output
 *     connection (the reference's behaviour; default for a 1-stream engine);
 *   - a tick runs when min_batch streams are ready (0: all connected ones), or max_wait_us after the first became ready
 *     (ragged batches: only the ready streams are stepped), but never sooner than the pacing rule allows (target_util_pct:
 *     small back-to-back batches would keep the GPU 100 % busy at its least efficient operating point);
 *   - output sockets are non-blocking like the reference's (:346-347): a listener that cannot take a whole packet is dropped;
 *   - a stream whose results are not finite (VAPX_OUT_STATUS) is reset and skipped for that tick, the others are served.
 * The engine handle must outlive the front-end and must not be stepped by anyone else while it runs. */
typedef struct vapx_ingest* vapx_ingest_handle;

typedef struct vapx_ingest_config {
  int32_t struct_size;      /* sizeof(vapx_ingest_config) */
  int32_t port_in;          /* 50007 in the reference (vap_main.py:470); 0 = ephemeral, see vapx_ingest_ports; -1 (both ports) = passive
                               shard of a vapx_frontdoor: no listening sockets of its own */
  int32_t port_out;         /* 50008 */
  int32_t rx_threads;       /* 0 = 2 */
  int32_t tx_threads;       /* 0 = 2 */
  int32_t max_wait_us;      /* 0 = 2000 */
  int32_t min_batch;        /* 0 = every connected stream */
  int32_t reset_on_connect; /* 1 = a new input connection starts from a fresh stream state */
  int32_t broadcast;        /* -1 = auto (1 for a single-stream engine), 0, 1 */
  int32_t bind_any;         /* 0 = 127.0.0.1 like the reference, 1 = 0.0.0.0 */
  double gain;              /* audio_gain, 1.0 = off */
  int32_t target_util_pct;  /* pacing: the next tick starts no earlier than (previous tick's start + its duration * 100 / pct), so the
                               engine stays at most pct % busy and batches grow instead of the queue (0 = 90; 100 = back-to-back) */
  int32_t flags;            /* VAPX_INGEST_* (0 = defaults) */
  /* thread placement (optional; a caller that passes the shorter struct of ABI 2 as first shipped gets 0 / 0 = no pinning): with
     cpu_count > 0 the front-end pins its threads to the cores cpu_first .. cpu_first + cpu_count - 1 (wrapping): tick (and accept) thread on
     the first, then one core per receive thread, then one per sender thread.  Give the cores of the GPU's NUMA node, and keep load
     generators / other tenants off them: with 4096 connections the kernel's softirq work for the sockets otherwise lands on whatever core a
     front-end thread happens to run on and its tail latency follows the neighbours'. */
  int32_t cpu_first;
  int32_t cpu_count;
  /* wire format of the input port (optional; a caller that passes a shorter struct gets 0): 0 = the reference's framing, 160 x {f64 ch1, f64 ch2}
     per 10 ms, cast to f32 on the host; VAPX_PCM_S16 / _MULAW / _ALAW = 10 ms packets of in_hz / 100 interleaved (ch1, ch2) sample pairs in that
     format (640 bytes s16 or 320 bytes G.711 at 16 kHz, 160 bytes G.711 at 8 kHz), de-interleaved into the staging as they are and decoded by
     the engine (vapx_set_input_format).  The result packet is unchanged: its x1 / x2 blocks carry the decoded samples as f64.  With an engine the
     format is the engine's and this field must be 0 or equal to it; the _fn variants take it from here.  gain != 1 with a raw format is refused. */
  int32_t input_format;
  /* input classes (optional; a caller that passes a shorter struct - up to and including input_format - gets 0 = no classes): one INPUT PORT PER
     CLASS in front of an engine with a class table (vapx_set_input_classes).  A connection accepted on class c's port takes the lowest free
     slot; the front-end calls vapx_set_stream_class(slot, c) and then receives that class's 10 ms packets: f64 pairs cast on the host for
     VAPX_PCM_F32 (the reference's framing), raw interleaved pairs de-interleaved as they are for s16 and G.711 (the sizes documented at
     input_format).  The tick packs the ready streams' slots into page-locked staging in batch order: the packed block of "Input classes".
     Result packets, output ports and the pairing of output connections to streams are unchanged; the echo carries the stream's decoded hop_in
     samples as f64, as a uniform front-end of that class sends them.  With an engine the table is the engine's: the config's must be empty
     (n_input_classes = 0) or equal to it; the _fn variant takes it from here.  class_ports_in[c] is the input port of class c (0 = ephemeral,
     see vapx_ingest_class_ports); port_in is ignored when a table is present.  Refused: input_format != 0 or gain != 1 with a raw class; a
     passive shard (port_in = -1), vapx_ingest_open_group* and therefore the front door: multi-port groups and doors are not part of this. */
  int32_t n_input_classes;
  vapx_input_class input_classes[VAPX_MAX_INPUT_CLASSES];
  int32_t class_ports_in[VAPX_MAX_INPUT_CLASSES];
  /* PAIR PORTS (struct_size = the whole struct; every earlier size, the one that ended with class_ports_in included, means "no pair ports"):
     input ports for dialogues whose two legs arrive in different classes of the table ("Input classes", CHANNEL CLASSES): a media gateway
     that forks an agent leg (48 kHz s16) and a customer leg (8 kHz G.711) sends both on ONE connection.  A connection accepted on pair port
     p takes the lowest free slot; the front-end calls vapx_set_stream_channel_classes(slot, cls_ch1, cls_ch2) and then receives PLANAR
     10 ms packets: channel 1's 10 ms in cls_ch1's wire form (input_hz / 100 samples: f64 for VAPX_PCM_F32, cast on the host; raw s16 /
     G.711 otherwise), followed by channel 2's 10 ms in cls_ch2's.  Samples cannot be interleaved across rates; a pair port takes planar
     packets also where cls_ch1 == cls_ch2.  A connection that ends inside a frame loses that part of a frame, as on every port.  Result
     packets keep their framing: x1 carries hop_in(cls_ch1) decoded samples and x2 hop_in(cls_ch2), each block with its own count.  The
     tick packs such a slot as the engine takes it: channel 1's row, then channel 2's.  Pair ports need a table (the engine's, or
     input_classes here); what a table refuses (a passive shard, a group, a gain with a raw class) stays refused.  port_in: 0 = ephemeral,
     see vapx_ingest_pair_ports. */
  int32_t n_pair_ports;                  /* 0 .. VAPX_MAX_PAIR_PORTS */
  struct { int32_t cls_ch1, cls_ch2, port_in; } pair_ports[16];
} vapx_ingest_config;
#define VAPX_MAX_PAIR_PORTS 16
#define VAPX_INGEST_CORE_SET 2      /* with cpu_count > 0: every front-end thread may run on ANY core of the range (one affinity set) instead of
                                       one core each: keeps other processes' work off the range without nailing a thread to a core that the
                                       kernel then borrows for softirq work */
#define VAPX_INGEST_KEEP_STATE 4    /* the engine's streams hold imported state (vapx_import_streams): vapx_ingest_open / _open_group skip their warm-up, which
                                       steps the first max_batch streams on silence and then resets them.  Step the engine once BEFORE importing
                                       instead (the first vapx_step of a process loads the code objects: hundreds of ms).  Combine with
                                       reset_on_connect = 0, or the first connection on a slot clears what was imported */
#define VAPX_INGEST_KEEP_NOFILE 1   /* never touch RLIMIT_NOFILE.  Default (flag clear): vapx_ingest_open* needs one descriptor per dialogue
                                       and one per listener; if the process's SOFT limit is below 2 x streams + 256 it is raised towards the
                                       hard limit with setrlimit() — a process-wide change the host should know about (select()-based code
                                       with FD_SETSIZE tables must not be handed descriptors >= 1024) */

typedef struct vapx_ingest_stats {
  int64_t frames_done;      /* stream-frames stepped and answered */
  int64_t ticks;            /* vapx_step calls */
  int64_t rx_bytes, tx_bytes;
  int64_t in_connections, out_connections;   /* currently open */
  int64_t dropped_listeners;                 /* output connections closed because they could not take a packet */
  int64_t numeric_resets;                    /* streams reset after non-finite results */
  int64_t overruns;                          /* frames a sender delivered faster than the engine consumed (input paused) */
  double mean_batch;                         /* streams per tick */
  double lat_mean_ms, lat_p50_ms, lat_p99_ms, lat_max_ms;   /* frame complete on the host -> result packet handed to the kernel */
  double step_mean_ms;                       /* time inside vapx_step per tick */
} vapx_ingest_stats;

int vapx_ingest_open(vapx_handle engine, const vapx_ingest_config* cfg, vapx_ingest_handle* out);
/* The same front-end over a caller-supplied step function instead of an engine (host-logic tests without a GPU):
 * step(user, n, stream_ids, audio[n][2][hop], out[n][VAPX_OUT_STRIDE]) returns 0 or a negative VAPX_E_* code;
 * reset(user, stream_id) may be NULL.  With cfg->input_format S16 / MULAW / ALAW `audio` points to the raw samples [n][2][hop] of that
 * format (the type stays const float*), exactly as an engine with that input format takes them. */
typedef int (*vapx_ingest_step_fn)(void* user, int32_t n, const int32_t* stream_ids, const float* audio, float* out);
typedef void (*vapx_ingest_reset_fn)(void* user, int32_t stream_id);
int vapx_ingest_open_fn(vapx_ingest_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                        int32_t frame_hz, int32_t mode, const vapx_ingest_config* cfg, vapx_ingest_handle* out);
int vapx_ingest_ports(vapx_ingest_handle g, int32_t* port_in, int32_t* port_out);   /* (0, 0) for a passive shard */
/* A front-end with input classes.  vapx_ingest_class_ports: the bound input port of every class (at most max), returns the number of classes
 * (0 without a table); vapx_ingest_ports then reports class 0's as port_in.  vapx_ingest_stream_class: for the step function of the _fn
 * variant, which receives the packed block exactly as an engine would - slot k of the batch holds [2][hop_in(c_k)] samples of format(c_k), c_k =
 * vapx_ingest_stream_class(g, stream_ids[k]), at the byte offset the earlier slots add up to; valid inside the step function (the tick
 * thread owns the answer); VAPX_E_INVAL without a table, VAPX_E_RANGE for a bad id. */
int32_t vapx_ingest_class_ports(vapx_ingest_handle g, int32_t* ports, int32_t max);
int32_t vapx_ingest_stream_class(vapx_ingest_handle g, int32_t stream_id);
/* Pair ports (vapx_ingest_config.pair_ports).  vapx_ingest_pair_ports: the bound input port of every pair port (at most max), returns their
 * number.  vapx_ingest_stream_channel_classes: out[0], out[1] = the classes of the stream's two channels, for the step function of the _fn
 * variant: slot k of its packed block holds channel 1's row, hop_in(out[0]) samples of format(out[0]), then channel 2's row of out[1]'s;
 * valid inside the step function.  vapx_ingest_stream_class answers VAPX_E_INVAL for a stream whose two classes differ. */
int32_t vapx_ingest_pair_ports(vapx_ingest_handle g, int32_t* ports, int32_t max);
int vapx_ingest_stream_channel_classes(vapx_ingest_handle g, int32_t stream_id, int32_t out[2]);
/* One front-end for a trunk group (vapx_attach_trunk): the reference's deployment of vap_main.py, vap_bc_main.py and vap_nod_main.py
 * side by side on one cpc_model file, with ONE input port and the audio encoded once.
 *   - input: cfg->port_in; every accepted connection is a dialogue exactly as with vapx_ingest_open (lowest free slot, carry re-zeroed,
 *     reset_on_connect, gain, overrun pause);
 *   - output: one port per model — the leader's is cfg->port_out, follower i's is follower_ports_out[i] (0 = ephemeral; NULL = all
 *     ephemeral).  A connection on model m's port hears model m's packets only, in that model's framing (vap util.py:122-143, bc
 *     :193-211, nod :213-237 with p_bc of every window row); fewest-listeners / lowest-slot placement and broadcast hold per port;
 *   - a tick is one vapx_step_group (host in, host out, page-locked wire block); batching, max_wait_us, pacing and min_batch are
 *     unchanged, and a stream's packets leave through one sender thread, so they stay in frame order on every port;
 *   - a stream with status 1 (not finite) in ANY model is reset through the leader (which resets the followers) and gets no packet on
 *     any port that tick; numeric_resets counts it once;
 *   - a mixed group (models with windows / rates of their own, read from each engine's vapx_get_config): input framing, ticks and
 *     batching stay the leader's.  A model at 1/R of the leader's rate sends ONE packet per R leader hops of a dialogue, echoing
 *     n = R * hop samples per channel as its reference program does (10 Hz: 1600, util.py:213-237): the front-end keeps an f64 echo
 *     history of R - 1 leader hops per dialogue, appended when the model's wire row carries VAPX_STATUS_NO_FRAME — which sends no
 *     packet on that model's port, resets nothing and is not a numeric_reset.  The history is cleared with the slot's carry on a new
 *     connection; without reset_on_connect the engine's phase runs on across the reconnect (as the reference's model state does), so
 *     a connection that starts in the middle of a slower model's frame gets no packet for that one frame;
 *   - stats: frames_done counts stream-frames (not packets), the latency of a stream-frame is taken once, after the LAST model's packets
 *     were handed to the kernel; tx_bytes, out_connections and dropped_listeners sum over the ports.
 * `followers` must be the leader's attached followers in attach order (modes pairwise distinct).  A group cannot be a passive shard:
 * port_in = -1 is refused (VAPX_E_INVAL, message in vapx_ingest_last_open_error); the front door stays single-model.
 * vapx_ingest_group_ports: the input port and up to max_ports output ports in model order; returns the number of models.
 * vapx_ingest_ports reports the leader's output port. */
int vapx_ingest_open_group(vapx_handle leader, const vapx_handle* followers, int32_t n_followers, const vapx_ingest_config* cfg,
                           const int32_t* follower_ports_out, vapx_ingest_handle* out);
int vapx_ingest_group_ports(vapx_ingest_handle g, int32_t* port_in, int32_t* ports_out, int32_t max_ports);
/* The same over a caller-supplied step function (host-logic tests without a GPU): step(user, n, stream_ids, audio[n][2][hop], wire_out)
 * fills wire_out in the layout of vapx_step_group for that tick's n and modes[0 .. n_models); ctx_frames sizes nod's wire rows.
 * vapx_ingest_open_group_fn2 takes every model's rate and window (frame_hzs[n_models], ctx_frames[n_models]; model 0 leads and is the
 * fastest, its rate an integer multiple of the others'): the step function then marks a slower model's rows without a frame with
 * VAPX_STATUS_NO_FRAME.  vapx_ingest_open_group_fn is fn2 with equal rates and windows.
 * vapx_ingest_last_open_error: why the calling thread's latest vapx_ingest_open_group* call was refused ("" if it was not). */
typedef int (*vapx_ingest_group_step_fn)(void* user, int32_t n, const int32_t* stream_ids, const float* audio,
                                         float* wire_out /* layout of vapx_step_group */);
int vapx_ingest_open_group_fn(vapx_ingest_group_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                              int32_t frame_hz, int32_t ctx_frames, const int32_t* modes, int32_t n_models, const vapx_ingest_config* cfg,
                              const int32_t* follower_ports_out, vapx_ingest_handle* out);
int vapx_ingest_open_group_fn2(vapx_ingest_group_step_fn step, vapx_ingest_reset_fn reset, void* user, int32_t n_streams, int32_t max_batch,
                               const int32_t* frame_hzs, const int32_t* ctx_frames, const int32_t* modes, int32_t n_models,
                               const vapx_ingest_config* cfg, const int32_t* follower_ports_out, vapx_ingest_handle* out);
const char* vapx_ingest_last_open_error(void);
int vapx_ingest_stats_read(vapx_ingest_handle g, vapx_ingest_stats* out, int32_t reset_latency_window);
/* Exact server-side count of late answers in the current latency window (since the last stats_read(.., 1)): result packets handed to the
 * kernel more than 10 ms after their frame was complete on the host — the north-star bound — and the packets of the window. */
int vapx_ingest_late_read(vapx_ingest_handle g, int64_t* over_10ms, int64_t* answered);
void vapx_ingest_close(vapx_ingest_handle g);

/* ---- one front door for N GPUs -----------------------------------------------------------------------------------------------------
 * The reference serves ONE port pair (proc_serv_in / proc_serv_out_dist bind port_num_in / port_num_out, vap_main.py:338-366,470-471).
 * For N GPUs in one process: create one engine per device (vapx_create, device_id = r), open one PASSIVE front-end per engine
 * (vapx_ingest_config.port_in = port_out = -1: it listens on nothing) and put them behind vapx_frontdoor_open, which owns the single
 * port pair and hands every accepted connection to a shard.  Dialogue slots are numbered globally g = local_slot * N + shard:
 *   - an input connection takes the lowest free global slot (GPUs fill evenly; a dialogue that reconnects while its slot is still the
 *     lowest free one returns to the GPU that holds its state);
 *   - the k-th output connection hears the k-th dialogue (fewest listeners, lowest global slot), as with a single front-end.
 * All shards must have the same frame rate and mode.  Close the front door first, then the shards, then the engines. */
typedef struct vapx_frontdoor* vapx_frontdoor_handle;
int vapx_frontdoor_open(vapx_ingest_handle* shards, int32_t n_shards, int32_t port_in, int32_t port_out, int32_t bind_any,
                        vapx_frontdoor_handle* out);
/* The same door with every shard in a process OF ITS OWN (one process per GPU: the process that owns the engine also owns its front-end's
 * threads and descriptors - a container's RLIMIT_NOFILE of 20 000 holds ~9 800 dialogues, BASELINE config 4 has 32 768).  Door and worker are
 * joined by one AF_UNIX / SOCK_SEQPACKET socket pair (`link`), created by whoever starts the workers:
 *   worker process:  vapx_create, vapx_ingest_open (passive: port_in = port_out = -1), vapx_ingest_attach_link(front_end, its end of the link)
 *   door process:    vapx_frontdoor_open_links(the other ends, n, port_in, port_out, ...) - it waits for every worker's greeting (slots, frame
 *                    rate, mode), then owns the reference's ONE port pair (vap_main.py:338-366,470-471)
 * The door keeps a mirror of every shard's slot / listener occupancy and is the only allocator: it names the slot, passes the accepted socket to
 * the worker (SCM_RIGHTS) and closes its own copy; workers report released slots and dropped listeners back over the link.  Placement is the
 * in-process door's: lowest free global slot g = local_slot * N + shard for inputs, fewest listeners / lowest global slot for outputs.  A worker
 * that dies takes its dialogues with it and receives no new ones; the others keep serving.  The link descriptors stay the caller's: close them
 * after vapx_frontdoor_close / vapx_ingest_close. */
int vapx_ingest_attach_link(vapx_ingest_handle g, int32_t link_fd);
int vapx_frontdoor_open_links(const int32_t* link_fds, int32_t n_links, int32_t port_in, int32_t port_out, int32_t bind_any,
                              vapx_frontdoor_handle* out);
int vapx_frontdoor_ports(vapx_frontdoor_handle d, int32_t* port_in, int32_t* port_out);
int vapx_frontdoor_counts(vapx_frontdoor_handle d, int64_t* accepted_in, int64_t* accepted_out, int64_t* refused);
void vapx_frontdoor_close(vapx_frontdoor_handle d);

/* The wire codec on its own (byte-parity tests against the reference's util.py output, tests/golden/wire.npz).
 * decode: n_bytes (a multiple of 16) of input packets -> n_bytes / 16 samples per channel as the engine sees them (f32) and as
 * the result packet echoes them (f64, gain applied); either destination may be NULL.  Returns the sample count or < 0.
 * encode: one result packet INCLUDING the 4-byte length prefix for an output row of vapx_step; x1 / x2 = the frame's n
 * echoed samples; returns the packet size (or the size needed if dst is NULL / cap too small, nothing written). */
int64_t vapx_wire_decode_input(const uint8_t* bytes, size_t n_bytes, double gain, float* x1_f32, float* x2_f32, double* x1_f64,
                               double* x2_f64);
int64_t vapx_wire_encode_result(int32_t mode, double t, const double* x1, const double* x2, int32_t n, const float* out_row,
                                uint8_t* dst, size_t cap);

const char* vapx_last_error(vapx_handle h);
int32_t vapx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VAPX_H_ */
