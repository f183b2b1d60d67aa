/*
 * ofdmrx.h -- C ABI of the MI355X-native OFDM receive path (libofdmrx.so).
 *
 * Drop-in boundary.  The reference has no plugin / FFI layer;
 * its only seams are
 *   (1) the process boundary   decode OUTPUT INPUT [SKIP]       decode.cc:559-563
 *   (2) the in-process seam    Decoder<value,cmplx,rate>(uint8_t *out,
 *           DSP::ReadPCM<value> *pcm, int skip_count)            decode.cc:375
 *       which pulls samples with pcm->read()/channels()/rate()   decode.cc:297-298,590
 *       and leaves 5380 payload bytes in `out`, which main() descrambles
 *       and writes                                               decode.cc:608-617
 * This library replaces seam (2) for batches of independent frames: the caller
 * (the `decode` CLI, a batch driver, or a binding) reads the WAV body into
 * memory and hands over raw PCM; the library returns payload bytes plus a
 * per-frame result struct carrying every diagnostic the reference prints to
 * stderr (decode.cc:400-401,438,446,502-503,517-519,555) and every failure
 * cause (decode.cc:393,419,430,435,440,543).
 *
 * Conventions: plain C, no exceptions across the ABI.  Return value 0 = ok,
 * negative = API / HIP error (ofdmrx_strerror).  A frame that fails to decode
 * is DATA (result.status), never an API error.  All buffers are caller-owned.
 * A handle is not thread-safe: one handle per (host thread, GPU).
 */
#ifndef OFDMRX_H
#define OFDMRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDMRX_ABI_VERSION 1
/* Minor revisions keep every struct and signature of OFDMRX_ABI_VERSION 1 and add entry points or tighten a check:
 *   1: skip counts outside 0..OFDMRX_MAX_SKIP fail the call with OFDMRX_E_ARG (they used to be clamped)
 *   2: ofdmrx_set_esn0_rows, ofdmrx_list_decoded_frames, ofdmrx_debug_decode_cons, ofdmrx_config.flags bit 1 (OFDMRX_FLAG_SCL_ALWAYS);
 *      frames whose hard decisions already form a codeword are decided by a syndrome check (same outputs)
 *   3: ofdmrx_set_attempt_log (every preamble of a SKIP loop, decode.cc:390-448); frames the syndrome check leaves are
 *      list-decoded from a queue in full residencies of the decoder (same outputs); OFDMRX_TAP_CONS_RAW needs no flag, and the
 *      LLR / METRIC / LANE_MESG taps answer OFDMRX_E_UNSUPPORTED for a frame that never went through the list decoder
 *   4: ofdmrx_decode_batch_device delivers to pinned host memory when both output pointers are pinned host memory
 *   5: ofdmrx_sc_decided_frames, ofdmrx_get_sc_timing, ofdmrx_debug_sc_path, ofdmrx_last_chunk_first_frame, ofdmrx_config.flags bit 2
 *      (OFDMRX_FLAG_NO_SC); `samples` and the frame stride must be multiples of the sample FRAME size (2-channel input: of the I/Q pair);
 *      with pinned host outputs the optional Es/N0 rows and attempt log must be pinned host memory as well (else OFDMRX_E_ARG); frames
 *      with raw bit errors whose sign-following path provably is the list decoder's lane 0 are finished by a list-1 decode of
 *      that path (same outputs)
 *   6: ofdmrx_config.flags bit 3 (OFDMRX_FLAG_TWO_LANES): a device-entry call of four chunks or more runs its second half through a
 *      second pipeline beside the first (same outputs; the handle then holds the state of two pipelines); the list-1 pass takes whole
 *      residencies of its decoders and leaves the rest to the next chunk's run (same outputs)
 *   7: ofdmrx_decode_stream, ofdmrx_decode_stream_device (every preamble of one recording in one call), ofdmrx_debug_stream_edges;
 *      added within 1.7 (the minor number stays: a caller detects them by symbol): the live feed - ofdmrx_feed_begin, ofdmrx_feed_push,
 *      ofdmrx_feed_end, ofdmrx_feed_lag, ofdmrx_feed_resident_samples; many recordings in one call - ofdmrx_decode_streams,
 *      ofdmrx_decode_streams_device, ofdmrx_debug_streams_edges; a bank of live channels - ofdmrx_bank_begin, ofdmrx_bank_push,
 *      ofdmrx_bank_end, ofdmrx_bank_resident_samples, ofdmrx_bank_preambles, ofdmrx_bank_last_stage_ops
 *   8: ofdmrx_debug_polar_modes, ofdmrx_debug_decode_cons_modes (the single-stage test entries for every mode of the mode table)
 *   9: the three transmitter entries refuse a freq_off outside encode.cc:389's band with OFDMRX_E_ARG (they used to fold the
 *      carriers round Nyquist);
 *      added within 1.9 (the minor number stays: a caller detects it by symbol): the Watterson fading channel - ofdmrx_util_fading;
 *      the wideband front end - ofdmrx_util_channelize_taps, ofdmrx_util_channelize, ofdmrx_bank_begin_wideband,
 *      ofdmrx_bank_push_wideband; the wideband synthesizer - ofdmrx_util_synthesize; the wideband survey - ofdmrx_util_survey_window,
 *      ofdmrx_util_survey, ofdmrx_util_find_bands; the wideband front end at a rational decimation -
 *      ofdmrx_util_channelize_ratio_taps, ofdmrx_util_channelize_ratio, ofdmrx_bank_begin_wideband_ratio; the wideband synthesizer
 *      at a rational interpolation - ofdmrx_util_synthesize_ratio; the wideband front end on a channel grid (a polyphase filter bank) -
 *      ofdmrx_util_channelize_grid_taps, ofdmrx_util_channelize_grid, ofdmrx_bank_begin_wideband_grid; the wideband synthesizer on
 *      a channel grid (a polyphase synthesis bank) - ofdmrx_util_synthesize_grid, ofdmrx_util_synthesize_grid_chunk; the grid
 *      survey (per-slot power from the filter bank) - ofdmrx_util_survey_grid, ofdmrx_util_find_slots; the wideband front end on a
 *      channel grid at any ratio P / Q (a mixed-radix filter bank) - ofdmrx_util_channelize_grid_ratio_taps,
 *      ofdmrx_util_grid_ratio_slots, ofdmrx_util_channelize_grid_ratio, ofdmrx_bank_begin_wideband_grid_ratio; the wideband
 *      synthesizer on a channel grid at any ratio P / Q (a mixed-radix synthesis bank) - ofdmrx_util_synthesize_grid_ratio,
 *      ofdmrx_util_synthesize_grid_ratio_chunk; the grid survey at any ratio P / Q (per-slot power from the mixed-radix bank) -
 *      ofdmrx_util_survey_grid_ratio, ofdmrx_util_find_slots_ratio; the wideband front end for a real (one-channel) capture -
 *      ofdmrx_util_channelize_real, ofdmrx_bank_begin_wideband_real */
#define OFDMRX_ABI_MINOR 9

#define OFDMRX_PAYLOAD_BYTES 5380     /* decode.cc:587  data_len = 43040/8 */
#define OFDMRX_CODE_LEN 65536         /* decode.cc:309  code_order 16 */
#define OFDMRX_FRAME_SAMPLES 95200    /* one-frame file written by encode @ 8 kHz */
#define OFDMRX_MAX_LIST 8
#define OFDMRX_MAX_SKIP 64            /* largest SKIP count per frame (decode.cc:583-585,448); beyond it: OFDMRX_E_ARG */

/* sample formats of the PCM body (what DSP::ReadWAV accepts, decode.cc:576) */
enum { OFDMRX_FMT_S16 = 0, OFDMRX_FMT_U8 = 1, OFDMRX_FMT_F32 = 2 };

/* per-frame status: one value per exit of Decoder::Decoder */
enum {
	OFDMRX_OK = 0,
	OFDMRX_NO_SYNC = 1,        /* decode.cc:393-394  stream ended while searching */
	OFDMRX_OSD_ERROR = 2,      /* decode.cc:418-421 */
	OFDMRX_HEADER_CRC = 3,     /* decode.cc:429-432 */
	OFDMRX_BAD_MODE = 4,       /* decode.cc:434-437 (modes 6..13 are decoded) */
	OFDMRX_BAD_CALLSIGN = 5,   /* decode.cc:439-442 */
	OFDMRX_PAYLOAD_CRC = 6     /* decode.cc:542-545 */
};

/* API error codes */
enum {
	OFDMRX_E_ARG = -1, OFDMRX_E_NOMEM = -2, OFDMRX_E_HIP = -3, OFDMRX_E_NODEV = -4, OFDMRX_E_UNSUPPORTED = -5
};

#define OFDMRX_FLAG_KEEP_RAW_CONS 1
#define OFDMRX_FLAG_SCL_ALWAYS 2
#define OFDMRX_FLAG_NO_SC 4
#define OFDMRX_FLAG_TWO_LANES 8

typedef struct ofdmrx_handle ofdmrx_handle;

typedef struct {
	int32_t abi_version;       /* OFDMRX_ABI_VERSION */
	int32_t sample_rate;       /* 8000, 16000, 44100 or 48000: which Decoder<value,cmplx,rate> this handle is
	                            * (decode.cc:590-602); anything else: OFDMRX_E_UNSUPPORTED (decode.cc:603-605) */
	int32_t list_size;         /* SCL list = SIMD width of the reference build (decode.cc:164-169): 8 (AVX2, the
	                            * benchmarked configuration; 0 = 8) or 4 (the 128-bit build) */
	int32_t device;            /* HIP device ordinal */
	int32_t chunk_frames;      /* frames resident per pass (0 = default: 8192) */
	int32_t max_samples;       /* max samples per frame (0 = ofdmrx_frame_samples(sample_rate, 6)) */
	int32_t descramble;        /* 1 = XOR payload with Xorshift32 like main(), decode.cc:613-615 */
	int32_t flags;             /* bit 0 (OFDMRX_FLAG_KEEP_RAW_CONS, the name is historical): debug taps: run the list decoder for
	                            * every frame and keep its per-lane messages, so that OFDMRX_TAP_LLR / _METRIC / _LANE_MESG
	                            * exist for every frame with a header;
	                            * bit 1 (OFDMRX_FLAG_SCL_ALWAYS): run the list decoder for every frame.  Without either, a frame
	                            * whose channel hard decisions already form a codeword with a valid CRC-32 is finished by that
	                            * syndrome check - the list decoder's lane 0 provably is that codeword - with
	                            * identical payload, status, best_lane and bit_flips, and its LLRs are never written; a frame the
	                            * syndrome check leaves is decoded along its sign-following path alone (list size 1) and finished
	                            * there when that path provably is the list decoder's lane 0 (min over the information leaves of
	                            * fl(metric so far + |llr|) > the path's final metric) and its CRC-32 is zero - again
	                            * with identical payload, status, best_lane (0) and bit_flips; every other frame is list-decoded;
	                            * bit 2 (OFDMRX_FLAG_NO_SC): without that list-1 pass (syndrome check, then the list decoder);
	                            * bit 3 (OFDMRX_FLAG_TWO_LANES): cut a device-entry call of four chunks or more in two and run the second
	                            * half through a second pipeline beside the first (created on first use; it doubles the handle's device
	                            * state, about 18 GB at the default chunk).  For input in which most frames have raw bit errors (-20 dB:
	                            * +6 %, the README's multipath chain: +8 %; clean input: -1 %); wants GPU_MAX_HW_QUEUES=8 or more in the
	                            * environment before the HIP runtime starts.  OFDMRX_LANES=2 / =1 in the
	                            * environment overrides the flag */
	void *stream;              /* hipStream_t to run on, NULL = library-owned stream.  Batches longer than one chunk
	                            * also use library-owned streams for the list decoder and its finishing kernel (chunk
	                            * pipeline); the given stream waits for them, so work enqueued on `stream` after a
	                            * decode call sees the finished batch */
} ofdmrx_config;

/* mirrors the reference's stderr diagnostics */
typedef struct {
	int32_t status;            /* OFDMRX_OK ... */
	int32_t symbol_pos;        /* decode.cc:400 "symbol pos" (window coordinate) */
	int64_t sc_start;          /* stream index of the Schmidl-Cox symbol body, -1 if none */
	float cfo_rad;             /* decode.cc:399,401 coarse cfo, rad/sample */
	float cfo_fine;            /* decode.cc:501,503 finer cfo */
	float sfo_slope;           /* decode.cc:498 average Theil-Sen slope */
	int32_t oper_mode;         /* decode.cc:438 */
	uint64_t call_sign;        /* decode.cc:439-446, base-37 integer */
	int32_t best_lane;         /* decode.cc:532-541, -1 if no lane passed CRC-32 */
	int32_t bit_flips;         /* decode.cc:555: sign(LLR) != decoded bit over the payload positions.  LLRs are fp32 values
	                            * within the 1e-5 intermediate tolerance of a scalar build's; one that sits that close to
	                            * zero may carry either sign, so this diagnostic can differ by a count or two (observed:
	                            * +-2 in 0.3 % of the frames near the waterfall, never above it).  Far below the waterfall of
	                            * the HEADER (48 kHz frames with 5 % raw bit errors) one frame in 192 differed by 5: cfo_rad
	                            * differs in its last bits (1.5e-7 rad/sample), over 440 000 samples that is 0.07 rad of
	                            * carrier phase, which the Theil-Sen stage absorbs with different hard decisions for points
	                            * on a decision boundary; payload, lane and every other field were identical.  Round 4, 43 000
	                            * frames against the oracle: one frame (mode 7, -17 dB) differed by 9, its coarse cfo by
	                            * 2e-6 rad/sample - the same mechanism; mono input (its front end is a blocked scan, the
	                            * reference's a serial fp32 recurrence), 160 000 frames from -30 dB to the waterfall: beyond
	                            * +-2 in 0.05 % of the noisy frames, by up to 11 (21 where half the frames are lost);
	                            * nothing that is decided differed in any frame.  AT the waterfall (-15 / -14.5 dB, where
	                            * 38 % of the frames are lost) 4 of 65 536 frames differed from the scalar restatement in
	                            * something decided: sync position one sample apart (decode.cc:143's nearbyint on a
	                            * boundary), or the list decoder keeping / losing the right path an ulp apart.  The timing
	                            * tie also occurred once in 230 000 mono frames above the waterfall (same payload) */
	float esn0_db_last;        /* decode.cc:517-519, cumulative Es/N0 after the last row */
	int32_t n_sync_rejects;    /* falling edges rejected at decode.cc:140-145 */
} ofdmrx_frame_result;

/* hipEvent timings of the last decode call, milliseconds, summed over chunks.  In a pipelined (multi-chunk) call the
 * polar / finish spans run beside the Theil-Sen / LLR spans of the next chunk: the stage times then overlap and add up to
 * more than the wall time; TOTAL sums the per-chunk latencies (first kernel to last kernel of each chunk). */
enum {
	OFDMRX_T_FRONT = 0, OFDMRX_T_SYNC, OFDMRX_T_HEADER, OFDMRX_T_DEMOD, OFDMRX_T_THEILSEN,
	OFDMRX_T_LLR, OFDMRX_T_POLAR, OFDMRX_T_FINISH, OFDMRX_T_TOTAL, OFDMRX_T_COUNT
};
typedef struct {
	float ms[OFDMRX_T_COUNT];
	int32_t launches[OFDMRX_T_COUNT];   /* kernel launches per stage */
} ofdmrx_timing;

int ofdmrx_abi_version(void);
int ofdmrx_abi_minor(void);
const char *ofdmrx_strerror(int err);

/* replaces `new Decoder<value,cmplx,8000>` (decode.cc:592): allocates device
 * state, tables (frozen mask, twiddles, MLS kernels, BCH generator) once */
int ofdmrx_create(const ofdmrx_config *cfg, ofdmrx_handle **out);
void ofdmrx_destroy(ofdmrx_handle *h);

/*
 * Decode n_frames independent frames.  Frame f occupies
 * samples + f*frame_stride_bytes, samples_per_frame sample frames of
 * `channels` interleaved values (1 = real, 2 = analytic I/Q; decode.cc:578,298); `samples` and frame_stride_bytes are
 * multiples of the sample size (4 for 16-bit I/Q pairs), else OFDMRX_E_ARG.
 * skip_counts[f] (nullable) is decode.cc's SKIP argument (decode.cc:583-585,448): 0..OFDMRX_MAX_SKIP preambles to
 * pass over; a negative or larger count is OFDMRX_E_ARG (the reference would loop to the end of the stream).
 * payload_out: n_frames*5380 bytes, zeroed for failed frames (the reference
 * leaves them uninitialised, decode.cc:588).
 * HOST pointers; blocks until done.
 */
int ofdmrx_decode_batch(ofdmrx_handle *h, const void *samples, int sample_format, int channels,
	size_t samples_per_frame, size_t frame_stride_bytes, size_t n_frames,
	const int32_t *skip_counts, uint8_t *payload_out, ofdmrx_frame_result *results);

/* same with DEVICE pointers (inputs already resident in HBM); asynchronous on
 * the handle's stream.  d_payload_out / d_results are device buffers - or, both of them, PINNED HOST memory (hipHostMalloc, a
 * registered range; revision 1.4): then every chunk's payloads and records are copied out right behind the chunk, beside the
 * next chunk's kernels (frames the list decoder finishes in a later flush are delivered by its last kernel, straight into the
 * pinned arrays), and the batch is on the host when the handle's stream has drained - the host-pointer entry's output half
 * without its input half.  (Pageable host memory is refused: OFDMRX_E_ARG.)  d_skip_counts (nullable) is read back once on
 * the handle's stream before anything is enqueued (the counts steer the host loop), so it is ordered after earlier
 * work on that stream; that read-back is the call's only host synchronisation. */
int ofdmrx_decode_batch_device(ofdmrx_handle *h, const void *d_samples, int sample_format, int channels,
	size_t samples_per_frame, size_t frame_stride_bytes, size_t n_frames,
	const int32_t *d_skip_counts, uint8_t *d_payload_out, ofdmrx_frame_result *d_results);

/*
 * Stream decode (revision 1.7): every frame of ONE recording - n_samples sample frames of `channels` interleaved values, as a WAV
 * body holds them (`encode OUT ... file1 .. fileN` writes up to 4096 payloads back to back, a receiver records minutes) - in one
 * call.  Record k is what `decode OUT INPUT k` gives on the same samples: the payload and the result ofdmrx_decode_batch returns for
 * that stream with skip_counts = {k}.  Record k belongs to the (k+1)-th preamble the Schmidl-Cox search accepts (decode.cc:390-448);
 * a preamble whose header then fails is a record too (status OSD_ERROR .. BAD_CALLSIGN: the SKIP loop counts it).  sc_start is the
 * preamble's stream index, n_sync_rejects counts the rejected triggers from the start of the stream.
 * *n_preambles: the number of accepted preambles (the smallest k for which `decode` would report NO_SYNC); only
 * min(*n_preambles, max_frames) records are written (payload_out: 5380 bytes each, results: one each) and nothing past them.
 * payload_out / results may be NULL when max_frames is 0.  n_samples: 1 .. 0x7fffffff / 2; formats, channels, alignment and error
 * codes as ofdmrx_decode_batch.  The handle's flags hold (KEEP_RAW_CONS, SCL_ALWAYS, NO_SC; TWO_LANES is ignored), Es/N0 rows
 * (ofdmrx_set_esn0_rows) are written for each record; the attempt log is NOT written (each record is one preamble's outcome).
 * ofdmrx_get_timing, ofdmrx_last_chunk_first_frame, the stage taps (frame = record index relative to the last chunk),
 * ofdmrx_list_decoded_frames and ofdmrx_sc_decided_frames describe the call as they do a batch call; the stream-wide DC-blocker
 * pass of mono input is OFDMRX_T_FRONT, the scan and accept OFDMRX_T_SYNC.
 * The scan is tiled: its timing metric comes from window sums each tile of 4096 samples forms in double, where the
 * batch scan carries running sums from the start of the frame - the fp32 metric values agree but for a last-bit rounding on a
 * boundary (the reference's own serial fp32 sums differ from both by more).
 * HOST pointers; blocks until done.
 */
int ofdmrx_decode_stream(ofdmrx_handle *h, const void *samples, int sample_format, int channels, size_t n_samples,
	size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_preambles);
/* the same with the samples in DEVICE memory, on the handle's stream; outputs in device memory or, both of them, pinned host memory
 * (as ofdmrx_decode_batch_device).  The call reads the preamble count back to the host once, after the scan, to plan the records into
 * chunks: that is its one host synchronisation, so it cannot be captured into a graph.  (A stream with more falling edges of the
 * timing metric than the scan's edge buffer holds - about one per 2048 samples - is scanned once more after the buffer has grown.) */
int ofdmrx_decode_stream_device(ofdmrx_handle *h, const void *d_samples, int sample_format, int channels, size_t n_samples,
	size_t max_frames, uint8_t *d_payload_out, ofdmrx_frame_result *d_results, size_t *n_preambles);
/* test entry: the trigger logic of the stream scan (decode.cc:93-116, as tiles and a scan over them) on a caller-given timing
 * sequence of n values, with the thresholds and match_len of the handle's rate: the falling edges (t_edge), the first index of the
 * maximum of each run (t_max) and index_max; at most max_edges of them are written, *n_edges counts all.  HOST pointers. */
int ofdmrx_debug_stream_edges(ofdmrx_handle *h, const float *timing, size_t n, size_t max_edges,
	int64_t *t_edge, int64_t *t_max, int32_t *index_max, size_t *n_edges);

/*
 * Many recordings in one call (added within revision 1.7): n_streams recordings - a directory of WAV files, a bank of receiver
 * channels, a sweep over multi-frame streams; what ofdmrx_tx_encode_stream_device writes - scanned together and their records
 * decoded in shared chunks.  Recording s is n_samples[s] sample frames at samples + s * stream_stride_bytes; the lengths may
 * differ, a length of 0 is allowed (no records), and the bytes between the end of a recording and the next stride are never read.
 * The records of recording s are, byte for byte - payload and every byte of every ofdmrx_frame_result - what ofdmrx_decode_stream
 * returns for that recording alone, for 2-channel and for mono input, every format and rate, however the recordings are batched:
 * sc_start is an index into recording s, n_sync_rejects counts from its start, n_preambles[s] is its own count.  Mono input keeps
 * that because every recording runs with its own tile count (ofdmrx_decode_stream is this call with one recording): the DC blocker's scan over tiles
 * of 4096 samples composes per recording, in the order a call with that recording alone composes it, and the analytic signal is
 * formed in stretches on multiples of 7936 samples from that recording's position 0.
 * Packing: records in recording order, then preamble order; recording s contributes min(n_preambles[s], max_frames_per_stream)
 * records, first_record[s] (n_streams + 1 entries) is its first index in that order and first_record[n_streams] the total.  Only
 * the first max_records of the packed order are written and nothing past them is touched; first_record describes the uncapped
 * packing, so a caller sees what was cut.  payload_out / results may be NULL only when max_records is 0 (a count-only call).
 * Es/N0 rows (ofdmrx_set_esn0_rows): row block i belongs to packed record i.  The attempt log is not written, OFDMRX_FLAG_TWO_LANES
 * is ignored, the other flags hold; ofdmrx_get_timing, the stage taps, ofdmrx_list_decoded_frames and ofdmrx_sc_decided_frames
 * describe the call as for a stream call.
 * OFDMRX_E_ARG, before any device call: a NULL handle, samples, n_samples, n_preambles or first_record; n_streams outside 1 .. 65535;
 * a length above 0x7fffffff / 2; a stride that is not a multiple of the sample-frame size or is smaller than the longest recording;
 * a bad format or channel count; NULL outputs with max_records > 0; an open feed.
 * HOST pointers; blocks until done.
 */
int ofdmrx_decode_streams(ofdmrx_handle *h, const void *samples, int sample_format, int channels,
	size_t n_streams, size_t stream_stride_bytes, const size_t *n_samples, size_t max_frames_per_stream, size_t max_records,
	uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_preambles, size_t *first_record);
/* the same with samples, payload_out and results in DEVICE memory (both outputs may instead be pinned host memory, as for
 * ofdmrx_decode_batch_device); n_samples, n_preambles and first_record are HOST arrays.  One host synchronisation: the read-back of
 * all recordings' edge and preamble counts after the scan (not one per recording).  If a recording has more falling edges than its
 * share of the edge buffer, the buffer grows and the scan runs once more, as in ofdmrx_decode_stream_device. */
int ofdmrx_decode_streams_device(ofdmrx_handle *h, const void *d_samples, int sample_format, int channels,
	size_t n_streams, size_t stream_stride_bytes, const size_t *n_samples, size_t max_frames_per_stream, size_t max_records,
	uint8_t *d_payload_out, ofdmrx_frame_result *d_results, size_t *n_preambles, size_t *first_record);
/* test entry: ofdmrx_debug_stream_edges for n_streams timing sequences at once (sequence s: n[s] values, packed back to back in
 * `timing`) through the segmented trigger scan: nothing of a sequence's trigger state enters the next.  t_edge, t_max, index_max:
 * [n_streams][max_edges_per_stream], the first max_edges_per_stream edges of every sequence; n_edges[s] counts all.  HOST pointers. */
int ofdmrx_debug_streams_edges(ofdmrx_handle *h, const float *timing, size_t n_streams, const size_t *n, size_t max_edges_per_stream,
	int64_t *t_edge, int64_t *t_max, int32_t *index_max, size_t *n_edges);

/*
 * Live feed (added within revision 1.7): the same recording pushed block by block as it arrives, each record returned once its last
 * sample is in.  One feed per handle; HOST pointers; the calls block.  A feed is a bank (below) of one channel whose records come
 * without channel and index: the same driver and kernels serve both.
 *   begin   opens a feed of `channels` interleaved values of sample_format: position 0, record 0.
 *   push    n_samples more sample frames (0 is allowed); returns the records that have become due, in preamble order.
 *   end     the stream is over: the last partial tile is scanned with n = the samples fed and every pending preamble decoded with
 *           the samples past the end read as zero - what ofdmrx_decode_stream does for a frame the recording cuts off.
 * The records of every push and of end, concatenated, are the records ofdmrx_decode_stream returns for the concatenation of the
 * pushed samples, however the stream is cut into pushes: sc_start is the absolute stream index (64-bit: the length of a feed is not
 * limited, only what is resident), n_sync_rejects counts from the start of the feed, record k is the (k+1)-th accepted preamble.
 * 2-channel input: payloads and every byte of every ofdmrx_frame_result equal the one-call result (the scan's tiles stay on
 * absolute multiples of 4096 samples and form their sums themselves; the trigger is carried from push to push as the small discrete
 * state the one-call scan carries from tile to tile).  Mono input: the DC blocker's double-precision states are composed in another
 * order, so cfo_rad, cfo_fine, sfo_slope and esn0_db_last may differ within the 1e-5 of the intermediates and bit_flips as described
 * at ofdmrx_frame_result; everything decided is equal.
 * Due: records leave in preamble order.  A preamble whose header fails is due once the scan has passed its edge (the scan works on
 * complete tiles of 4096 samples) and its header symbol has arrived; one with a valid header once the last sample of the frame of
 * that header's mode has arrived - the end of its last symbol, sc_start + ofdmrx_frame_samples(rate, mode) - 2 rate -
 * (2 x 1440 + 160) rate / 8000 samples - plus ofdmrx_feed_lag(), which is 0: no kernel reads past the frame.
 * max_frames: at most that many records are written (payload_out: 5380 bytes each; NULL outputs only with max_frames 0) and
 * *n_records counts them; the rest stay staged in the handle, in order, *n_left counts those, and later push (n_samples may be 0) or
 * end calls return them.  The feed closes when an end call leaves *n_left == 0; begin then starts a new stream.  After the first
 * end call push accepts n_samples == 0 only.  Es/N0 rows (ofdmrx_set_esn0_rows, a host pointer): row block i belongs to the i-th
 * record the call writes.  The attempt log is not written and OFDMRX_FLAG_TWO_LANES is ignored, as for stream calls;
 * ofdmrx_get_timing and the stage taps describe the last decode a feed call ran.
 * OFDMRX_E_ARG: push / end without begin, begin while a feed or a bank is open, any ofdmrx_bank_*, ofdmrx_decode_batch* /
 * ofdmrx_decode_stream* while a feed is open, a NULL handle, NULL samples with n_samples > 0, NULL n_records / n_left, NULL outputs with max_frames > 0, a bad format
 * or channel count, samples not on a sample-frame boundary - all before any device call.  ofdmrx_destroy frees an open feed.
 * ofdmrx_feed_resident_samples: sample frames of the stream held on the device now: fed - base, where base is the largest multiple
 * of 4096 not above the smallest of
 *   scanned - BUFFER_LEN                      (scanned: the scan's frontier, the largest multiple of 4096 <= fed; BUFFER_LEN = 6 x 1440 rate / 8000)
 *   sc_start of the oldest preamble not yet decoded
 *   i_max - (MATCH_DEL + 4 x 1440 rate / 8000) while the trigger is on (i_max: the maximum of the timing metric in the running run)
 *   mono input: the start of the front-end stretch (7936 samples) that holds the last sample, minus 320
 * taken before a push appends its samples.  With at most one frame pending and the trigger's runs shorter than a frame it never
 * exceeds ofdmrx_frame_samples(rate, 13) + BUFFER_LEN + 3 x 4096 + the largest push so far; each further pending frame may add its
 * span.  (Device memory: two buffers of up to 1.5 x the largest window, the window moves from one to the other.)
 * -1 (OFDMRX_E_ARG) from either query without an open feed.
 */
int ofdmrx_feed_begin(ofdmrx_handle *h, int sample_format, int channels);
int ofdmrx_feed_push(ofdmrx_handle *h, const void *samples, size_t n_samples, size_t max_frames,
	uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_records, size_t *n_left);
int ofdmrx_feed_end(ofdmrx_handle *h, size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results,
	size_t *n_records, size_t *n_left);
long long ofdmrx_feed_lag(ofdmrx_handle *h);
long long ofdmrx_feed_resident_samples(ofdmrx_handle *h);

/*
 * Live feed bank (added within revision 1.7): many recordings that are all still arriving - a bank of receiver channels - pushed and
 * decoded in one call.  One bank per handle, never beside a feed; HOST pointers; the calls block.  A push costs the same number of
 * kernel launches, copies and host synchronisations whatever the number of channels, and the records that are due on all channels
 * go through the record pipeline together, in shared chunks.
 *   begin   n_channels (1 .. 65535) receiver channels, all of `channels` interleaved values of sample_format at the handle's rate;
 *           every channel starts at position 0, record 0.
 *   push    channel c brings n_samples[c] more sample frames (0 allowed; each <= 1 << 26), found at samples + c * stride_bytes.
 *           ends (nullable, [n_channels]): non-zero = channel c's stream is over after these samples.  Returns the records that
 *           have become due.
 *   end     every channel still open ends; the bank closes when an end call leaves *n_left == 0.
 * Per channel: the records of channel c are the records returned for c (record_channel[i] == c) over all push and end calls,
 * concatenated in the order returned.  They equal what a single ofdmrx_feed_* (a bank of that channel alone) returns when fed
 * channel c's samples in the same sequence of push lengths - every payload byte and every byte of every ofdmrx_frame_result, every format and every rate.  A
 * zero-length share counts as a zero-length push: the channel behaves as a single feed does with that push left out.  For 2-channel
 * input this is therefore also ofdmrx_decode_stream of the concatenation of channel c's samples, byte for byte.
 * Mono input inherits the feed's documented relation to the one-call decode and no more: every channel's DC-blocker states are
 * composed in exactly the order a single feed with that channel's push lengths composes them.
 * Positions and counters: sc_start is the absolute position in channel c (64-bit), n_sync_rejects counts from channel c's start,
 * record_index[i] is k, the preamble index ofdmrx_decode_stream would give the record, record_channel[i] is c.
 * Nothing crosses channels: how many other channels there are, what they hold, when they push and whether they have ended has no
 * effect on a channel's records.
 * Due: a channel's record is due by the single feed's rule applied to that channel's own samples fed and scan frontier - one with a
 * valid header once its frame's last sample has arrived, one with a failed header once the scan has passed its edge and its header
 * symbol has arrived.  A channel that ends has its last partial tile scanned with n = its samples fed and every pending preamble
 * decoded with the samples past the end read as zero, in the call that ends it.
 * Order: within one call the records are ordered by channel index, then by preamble order; across calls delivery is first in, first
 * out.  max_records caps what a call writes (payload_out: 5380 bytes each); the rest stay staged, *n_left counts them, and a later
 * call (all lengths 0) drains them.  Nothing past the first *n_records entries of any output array is touched.
 * Es/N0 rows (ofdmrx_set_esn0_rows, a host pointer): row block i belongs to the i-th record the call writes.  The attempt log is not
 * written and OFDMRX_FLAG_TWO_LANES is ignored; the other flags hold, as for the feed.
 * An ended channel accepts only n_samples[c] == 0 and stays closed until the bank closes.
 * OFDMRX_E_ARG, before any device call: push or end without begin; begin while a bank or a feed is open; any ofdmrx_feed_*,
 * ofdmrx_decode_batch* or ofdmrx_decode_stream* while a bank is open; a NULL handle, n_samples, n_records or n_left; NULL samples
 * while any length is non-zero; NULL outputs (any of the four arrays) with max_records > 0; n_channels outside 1 .. 65535; a bad
 * format or channel count; a length above 1 << 26; samples for an ended channel; a stride that is not a multiple of the
 * sample-frame size or is smaller than the longest share of this push; samples off the sample-frame boundary; a channel index out
 * of range in the two queries (they return -1).  ofdmrx_destroy frees an open bank.
 * ofdmrx_bank_resident_samples: as ofdmrx_feed_resident_samples, for one channel: fed[c] - base[c].  Device memory: the windows of
 * all channels share one capacity - two slabs of n_channels x cap sample frames, cap up to 1.5 x the largest window any channel has
 * needed, so 2 x cap x (bytes per sample frame) per channel (mono input: 2 x cap x (bytes per sample + 8 + 1 / 8) for the samples,
 * the analytic signal and the DC blocker's kept states) - plus 200 bytes of per-channel parameters and carries, every channel's
 * share of the edge buffer (at most 4096 edges of 40 bytes), and the packed new samples of one push.
 * ofdmrx_bank_preambles: preambles accepted on that channel so far.
 * ofdmrx_bank_last_stage_ops: kernel launches + memcpys + host synchronisations the bank's own stages (window move, new samples,
 * scan, accept, records, header) enqueued in the last bank call - NOT the record pipeline's (decode_records), whose count follows
 * the number of records.  It does not depend on n_channels; it grows only with an edge-buffer regrow pass and with the header
 * stage's loop over chunks when more preambles are pending than a chunk holds.
 */
int ofdmrx_bank_begin(ofdmrx_handle *h, size_t n_channels, int sample_format, int channels);
int ofdmrx_bank_push(ofdmrx_handle *h, const void *samples, size_t stride_bytes, const size_t *n_samples, const uint8_t *ends,
	size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, int32_t *record_channel, int64_t *record_index,
	size_t *n_records, size_t *n_left);
int ofdmrx_bank_end(ofdmrx_handle *h, size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results,
	int32_t *record_channel, int64_t *record_index, size_t *n_records, size_t *n_left);
long long ofdmrx_bank_resident_samples(ofdmrx_handle *h, size_t channel);
long long ofdmrx_bank_preambles(ofdmrx_handle *h, size_t channel);
long long ofdmrx_bank_last_stage_ops(ofdmrx_handle *h);

/*
 * Wideband bank (added within revision 1.9, detected by symbol): a bank whose channels are all cut from ONE wideband I/Q capture by
 * the wideband front end (ofdmrx_util_channelize below) on the device, as the capture arrives.
 *   begin_wideband  n_channels (1 .. 65535) channels centred at centre_hz[c] (a HOST array) of a capture at decim x the handle's
 *                   rate, arriving as interleaved I/Q of sample_format.  The channels are 2-channel F32 at the handle's rate.
 *   push_wideband   n_wide more wideband sample frames (0 allowed; <= 1 << 26; a HOST pointer).  After W frames in all every channel
 *                   has been fed ceil(W / decim) samples.  end != 0: every channel's stream is over after these samples.  The output
 *                   arguments are those of ofdmrx_bank_push.  The block is copied once, behind the last T - 1 wideband samples, and
 *                   one kernel launch writes every channel's new samples into its window.
 * ofdmrx_bank_end, ofdmrx_bank_resident_samples, ofdmrx_bank_preambles and ofdmrx_bank_last_stage_ops serve a wideband bank
 * unchanged; ofdmrx_bank_last_stage_ops stays independent of n_channels.
 * The contract: for every channel c and ANY cutting of the capture into pushes (lengths that are no multiple of decim, and zero,
 * included) the records of c equal what ofdmrx_decode_stream (F32, 2 channels) returns for row c of ofdmrx_util_channelize over the
 * whole capture - every payload byte and every byte of every ofdmrx_frame_result.  (The front end's outputs do not depend on where a
 * block boundary falls, and a bank channel equals the one-call decode of its samples.)  sc_start counts the channel's samples: the
 * front end's group delay puts it 12 samples behind the signal.
 * OFDMRX_E_ARG, before any device call: what ofdmrx_bank_begin and ofdmrx_bank_push refuse (an open feed or bank, NULL outputs with
 * max_records > 0, NULL samples with n_wide > 0, samples off the sample-frame boundary, samples after the end, ...); NULL centre_hz;
 * decim outside 2..32; a centre that is not finite or lies outside +- decim rate / 2; ofdmrx_bank_push on a wideband bank;
 * ofdmrx_bank_push_wideband on a plain bank; ofdmrx_util_channelize while any bank is open (a wideband bank owns the taps and
 * increments on the device).
 */
int ofdmrx_bank_begin_wideband(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int decim, int sample_format);
int ofdmrx_bank_push_wideband(ofdmrx_handle *h, const void *samples, size_t n_wide, int end, size_t max_records, uint8_t *payload_out,
	ofdmrx_frame_result *results, int32_t *record_channel, int64_t *record_index, size_t *n_records, size_t *n_left);
/* ... of a capture at p / q x the handle's rate (added within revision 1.9, detected by symbol): the front end
 * is ofdmrx_util_channelize_ratio below.  ofdmrx_bank_push_wideband, ofdmrx_bank_end and the queries serve it unchanged: after W
 * frames every channel has been fed ceil(W q / p) samples, one copy and one launch per push, and the contract above holds with row c
 * of ofdmrx_util_channelize_ratio.  OFDMRX_E_ARG: what ofdmrx_bank_begin_wideband refuses, with the ratio's limits in place of
 * decim's (p or q <= 0, reduced q above 16, p / q outside 2..32) and centres outside +- rate p / q / 2.  A ratio whose reduced q is 1
 * opens the bank ofdmrx_bank_begin_wideband opens. */
int ofdmrx_bank_begin_wideband_ratio(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int p, int q, int sample_format);
/* ... of a capture at decim x the handle's rate whose channels lie on the raster rate / 2 (added within revision 1.9, detected by
 * symbol): the front end is ofdmrx_util_channelize_grid below, decim a power of two 2 .. 512, channel j the
 * slot slots[j] (slots NULL with n_slots = 2 decim: every slot in ascending order).  ofdmrx_bank_push_wideband, ofdmrx_bank_end and
 * the queries serve it unchanged: one copy behind the kept tail (up to 24 decim = 12288 wideband samples) and one launch per push,
 * whatever the number of slots, and the contract above holds with row j of ofdmrx_util_channelize_grid.  OFDMRX_E_ARG: what
 * ofdmrx_bank_begin_wideband refuses, with a decim that is no power of two in 2..512, a slot outside -decim .. decim - 1 and n_slots
 * outside 1..65535 in the place of its limits.  While it is open ofdmrx_util_channelize* (the grid entry too) and ofdmrx_bank_push
 * are refused. */
int ofdmrx_bank_begin_wideband_grid(ofdmrx_handle *h, size_t n_slots, const int32_t *slots, int decim, int sample_format);
/* ... of a REAL capture at p / q x the handle's rate, one value of sample_format per wideband position (added within revision 1.9,
 * detected by symbol): the front end is ofdmrx_util_channelize_real below, q = 1 its integer decimation.
 * ofdmrx_bank_push_wideband, ofdmrx_bank_end and the queries serve it unchanged: n_wide counts real samples (samples on the
 * sample's boundary), after W of them every channel has been fed ceil(W q / p) samples, the tail kept between pushes is T - 1 samples,
 * one copy and one launch per push whatever the number of channels, and the contract above holds with row c of
 * ofdmrx_util_channelize_real.  OFDMRX_E_ARG: what ofdmrx_bank_begin_wideband_ratio refuses, with ofdmrx_util_channelize_real's rule
 * for the centres in place of "outside +- rate p / q / 2".  The plain and the wideband entries refuse each other as above, and
 * ofdmrx_util_channelize_real is refused while a feed or bank is open. */
int ofdmrx_bank_begin_wideband_real(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int p, int q, int sample_format);

int ofdmrx_synchronize(ofdmrx_handle *h);
int ofdmrx_get_timing(ofdmrx_handle *h, ofdmrx_timing *t);
int ofdmrx_chunk_frames(ofdmrx_handle *h);
/* A decode call runs its frames in chunks of at most ofdmrx_chunk_frames() frames - and a call whose outputs cross PCIe (the
 * host-pointer entry; the device entry with pinned host outputs) and whose 6144 or more frames fit ONE chunk runs as two halves
 * (the second half's kernels beside the first half's copies), unless the handle has OFDMRX_FLAG_KEEP_RAW_CONS.  The stage taps
 * below belong to the LAST chunk a call ran: this is the index, in that call, of the chunk's first frame (frame 0 of
 * ofdmrx_debug_dump).  Revision 1.5. */
long long ofdmrx_last_chunk_first_frame(ofdmrx_handle *h);
/* decode.cc:506-523 prints one Es/N0 value per constellation row.  rows = n_frames x OFDMRX_ROWS_MAX floats (dB; rows a frame's
 * mode does not have, and frames without a header: 0) in the memory space of the RESULTS of the decode calls that follow: a
 * device pointer for ofdmrx_decode_batch_device, a host pointer for ofdmrx_decode_batch.  NULL (the default) turns it off;
 * ofdmrx_frame_result.esn0_db_last always carries the last row's value. */
#define OFDMRX_ROWS_MAX 126    /* decode.cc:181 rows_max */
int ofdmrx_set_esn0_rows(ofdmrx_handle *h, float *rows);
/* frames of the last decode call that went through the list decoder; the rest were decided by the syndrome certificate
 * (see ofdmrx_config.flags).  -1 if the certificate is off for this handle.  Synchronises the handle's stream.
 * (The certificate is adaptive: after a chunk in which it was tried for 64 frames or more and finished fewer than one in twenty it
 * is tried for a sample of one frame in sixteen only, until a fifth of the sample - summed over chunks until eight frames have been
 * tried - passes again; a frame it was not tried for is list-decoded, with the same outputs.  Every call starts with the certificate on.) */
long long ofdmrx_list_decoded_frames(ofdmrx_handle *h);
/* frames of the last decode call that the list-1 pass finished (neither the syndrome check nor the list decoder); -1 if that
 * pass is off for this handle (OFDMRX_FLAG_KEEP_RAW_CONS / _SCL_ALWAYS / _NO_SC).  Synchronises the handle's stream.  The pass is
 * adaptive like the syndrome check: after a run of 64 entries or more of which it finished fewer than an eighth only a probe sample
 * goes through it - one frame in sixteen of every FOURTH chunk - until an eighth of the sample (summed over chunks until eight frames
 * have been tried) is finished again; the others go straight to the list decoder.  Default layout: one codeword per wave, ten resident
 * decoders per CU (OFDMRX_SC_LB / OFDMRX_SC_WPC in the environment change it); a run takes whole residencies of them and leaves the rest
 * to the next chunk's run (revision 1.6), the last run of a call takes everything. */
long long ofdmrx_sc_decided_frames(ofdmrx_handle *h);
/* hipEvent time and launches of that pass (k_sc + k_sc_finish) in the last decode call, like ofdmrx_timing's stages (which keep
 * their layout); either pointer may be NULL */
int ofdmrx_get_sc_timing(ofdmrx_handle *h, float *ms, int32_t *launches);
/* decode.cc:390-448 prints "symbol pos" / "coarse cfo" and the header's outcome for EVERY preamble the SKIP loop examines, not
 * only for the last one (which ofdmrx_frame_result describes).  log = n_frames x (OFDMRX_MAX_SKIP + 1) records, counts =
 * n_frames numbers of records written (0: the stream ended before any preamble), both in the memory space of the RESULTS of the
 * decode calls that follow (see ofdmrx_set_esn0_rows).  NULL, NULL (the default) turns it off. */
typedef struct {
	int32_t status;            /* OFDMRX_OK, or OFDMRX_OSD_ERROR .. OFDMRX_BAD_CALLSIGN: what decode.cc:417-442 made of this preamble */
	int32_t symbol_pos;        /* decode.cc:400 */
	float cfo_rad;             /* decode.cc:401 */
	int32_t oper_mode;         /* decode.cc:433 (valid from OFDMRX_BAD_MODE on) */
	uint64_t call_sign;        /* decode.cc:439 */
} ofdmrx_attempt;
int ofdmrx_set_attempt_log(ofdmrx_handle *h, ofdmrx_attempt *log, int32_t *counts);

/* ---- stage taps for parity tests (host destination buffers) --------------
 * Valid for frames of the LAST chunk processed (frame index relative to that
 * chunk's first frame, ofdmrx_last_chunk_first_frame()).  The rotated constellation is made on demand (the pipeline never stores it); LLR / METRIC /
 * LANE_MESG exist for frames that went through the list decoder (every frame with a header when the handle was created with
 * OFDMRX_FLAG_KEEP_RAW_CONS or OFDMRX_FLAG_SCL_ALWAYS; LANE_MESG needs the former), otherwise: OFDMRX_E_UNSUPPORTED. */
enum {
	OFDMRX_TAP_HDR_SOFT = 1,   /* int8  [255]      decode.cc:413-416 */
	OFDMRX_TAP_CONS_RAW = 2,   /* cf32  [cons_cnt <= 32400] decode.cc:464-477 (21600 in mode 6) */
	OFDMRX_TAP_CONS_ROT = 3,   /* cf32  [cons_cnt]          decode.cc:481-495 */
	OFDMRX_TAP_SLOPE = 4,      /* f32   [rows <= 126]       (50 in mode 6) */
	OFDMRX_TAP_YINT = 5,       /* f32   [rows] */
	OFDMRX_TAP_PRECISION = 6,  /* f32   [rows]              decode.cc:517 */
	OFDMRX_TAP_LLR = 7,        /* f32   [65536]    decode.cc:529 */
	OFDMRX_TAP_METRIC = 8,     /* f32   [8] */
	OFDMRX_TAP_LANE_MESG = 9,  /* u8    [8][5476]  systematic message bits per lane, LE packed: the first 5476 bytes of every lane (all of
	                            *                   them in modes 6-9; modes 10-13 have 5512: ofdmrx_debug_polar_modes returns [8][5512]) */
	OFDMRX_TAP_ANALYTIC = 10   /* cf32  [samples]  after D1 (mono only) */
};
int ofdmrx_debug_dump(ofdmrx_handle *h, int tap, size_t frame, void *dst, size_t dst_bytes);

/* ---- single-stage entry points for parity tests (HOST pointers) ---------- */
/* D9+D10: CODE::PolarListDecoder + systematic() (decode.cc:530-531) */
int ofdmrx_debug_polar(ofdmrx_handle *h, const float *llr /*n*65536*/, size_t n,
	uint8_t *lane_mesg /*n*8*5476*/, float *metric /*n*8*/);
/* the same for any mode of the mode table: vector i is a codeword of mode oper_modes[i] (6..13, else OFDMRX_E_ARG; NULL: all mode
 * 6), which decides its frozen table and message length; neighbours i, i + 1 of the same table are decoded as a pair by a
 * list_size 4 handle.  Every lane's message comes back complete: mesg_bits / 8 bytes (5476 in modes 6-9, 5512 in modes 10-13),
 * zero-padded to 5512. */
int ofdmrx_debug_polar_modes(ofdmrx_handle *h, const float *llr /*n*65536*/, size_t n, const int32_t *oper_modes /*n*/,
	uint8_t *lane_mesg /*n*8*5512*/, float *metric /*n*8*/);
/* the sign-following path of the list decoder alone (k_sc): n LLR vectors, vector i of the code of mode oper_modes[i] (NULL: all
 * mode 6) -> its re-encoded codeword (bit i = bit i % 8 of byte i / 8), the hard decisions of the LLRs packed alike, its path
 * metric, min over the information leaves of fl(metric so far + |llr|), and whether the rule "min_fork > metric, every |llr| <
 * 6e29" holds.  Any output may be NULL. */
int ofdmrx_debug_sc_path(ofdmrx_handle *h, const float *llr /*n*65536*/, size_t n, const int32_t *oper_modes /*n*/,
	uint8_t *codeword /*n*8192*/, uint8_t *hard /*n*8192*/, float *metric /*n*/, float *min_fork /*n*/, int32_t *rule_ok /*n*/);
/* D5 output (n x 21600 rotated constellation points of mode-6 frames, cf32) -> payloads + results through D6-D10 as the pipeline
 * chains them: use_cert 0 = the list decoder for every frame, 1 = the syndrome certificate in front of it, 2 = syndrome certificate,
 * list-1 pass, list decoder (the default chain), 3 = list-1 pass, list decoder; cert_out (nullable): 1 = the frame was finished
 * by the syndrome certificate, 2 = by the list-1 pass, 0 = by the list decoder (decode.cc:505-555) */
int ofdmrx_debug_decode_cons(ofdmrx_handle *h, const float *cons /*n*21600*2*/, size_t n, int use_cert,
	uint8_t *payload /*n*5380*/, ofdmrx_frame_result *results /*n*/, int32_t *cert_out /*n*/);
/* the same for any mode of the mode table: frame i is of mode oper_modes[i] (6..13, else OFDMRX_E_ARG; NULL: all mode 6) and
 * supplies that mode's cols x rows rotated points (<= 32400) at cons + i * cons_stride_points (a stride smaller than a frame's
 * point count: OFDMRX_E_ARG); results[i].oper_mode is oper_modes[i].  Frames of all modes may share a call: the list-1 pass and
 * the list decoder's queue then hold both frozen tables. */
int ofdmrx_debug_decode_cons_modes(ofdmrx_handle *h, const float *cons /*n*cons_stride_points*2*/, size_t cons_stride_points, size_t n,
	const int32_t *oper_modes /*n*/, int use_cert, uint8_t *payload /*n*5380*/, ofdmrx_frame_result *results /*n*/, int32_t *cert_out /*n*/);
/* DSP::TheilSenEstimator::compute on rows of y[cols], x = i - cols/2 (decode.cc:488) */
int ofdmrx_debug_theil_sen(ofdmrx_handle *h, const float *y, size_t rows, int cols,
	float *slope, float *yint);
/* CODE::OrderedStatisticsDecoder<255,71,4> (decode.cc:417): soft n*255 -> hard n*32 (BE bits), unique n */
int ofdmrx_debug_osd(ofdmrx_handle *h, const int8_t *soft, size_t n, uint8_t *hard, int32_t *unique);
/* DSP::FastFourierTransform<1280|640,cmplx,-1|+1> (decode.cc:191,43-44): n transforms */
int ofdmrx_debug_fft(ofdmrx_handle *h, const float *in, size_t n, int len, int sign, float *out);

/* ---- build-owned channel model on device (aicodix/disorders is absent) ----
 * out frame f = base frame (f % n_base) + complex AWGN of power 10^(noise_db/10)
 * (re/im split equally), counter-based RNG keyed by (seed, first_frame+f).
 * 2-channel int16 in and out, DEVICE pointers, samples_per_frame each.
 * In place is allowed in one form only: d_out == d_base with n_out <= n_base, where frame f reads and writes only itself.
 * Any other overlap of the two buffers, and a noise_db that is not finite, is OFDMRX_E_ARG.  What pins the noise to its
 * definition, sample by sample: DESIGN.md section 4.8. */
int ofdmrx_util_awgn_tile(ofdmrx_handle *h, const int16_t *d_base, size_t n_base,
	int16_t *d_out, size_t n_out, size_t samples_per_frame, float noise_db,
	uint64_t seed, uint64_t first_frame);

/* deterministic part of the README.md:49 chain (multipath | cfo | sfo), applied to n 2-channel int16 frames on the
 * device (n <= 65535); ofdmrx_util_awgn_tile then adds the independent noise.  Definitions: DESIGN.md / oracle/channel.c */
typedef struct {
	float cfo_hz;              /* carrier frequency offset, Hz (at the handle's sample rate) */
	float sfo_ppm;             /* sampling frequency offset, ppm */
	int32_t ntaps;             /* multipath taps (0..8); 0 = pass-through */
	int32_t delays[8];         /* samples */
	float gains_re[8], gains_im[8];
} ofdmrx_channel;
/* delays must lie in [0, samples_per_frame); d_in and d_out must not overlap (else OFDMRX_E_ARG) */
int ofdmrx_util_channel(ofdmrx_handle *h, const int16_t *d_in, int16_t *d_out, size_t n_frames,
	size_t samples_per_frame, const ofdmrx_channel *ch);

/* Watterson / ITU-R F.520 fading channel (added within revision 1.9), a new realisation per frame: out frame f is in frame
 * (f % n_in) - the tiling of ofdmrx_util_awgn_tile, so one transmission can be reused under many fades - through ntaps paths
 * whose gains are complex Gaussian processes with a Gaussian Doppler spectrum of frequency spread (2 sigma) spread_hz[t] and
 * mean power |gain|^2, realised by the sum-of-sinusoids method as closed forms of (seed, first_frame + f, sample index): DESIGN.md
 * section 4.13 is the definition, held sample by sample.  The same seed gives fading that is independent of the noise of
 * ofdmrx_util_awgn_tile.  A path with spread_hz == 0 is specular: its gain is the constant `gain`.  No per-path Doppler shift: a
 * common shift is ofdmrx_channel.cfo_hz.  2-channel int16 in and out, DEVICE pointers, asynchronous on the handle's stream.
 * OFDMRX_E_ARG, before any device call: NULL pointers or zero counts; ntaps outside 1..8; a delay that is negative, >=
 * samples_per_frame or above OFDMRX_FADING_MAX_DELAY; a gain or spread that is not finite; a spread outside 0 .. rate / 800 (the
 * gain is interpolated linearly between knots OFDMRX_FADING_KNOT samples apart, which holds while the phase advance per knot stays
 * well below a radian); ANY overlap of the two buffers (paths read neighbouring samples: there is no in-place form); what the
 * launch cannot hold: n_out above 2^31 - 1, samples_per_frame above 65535 * 4096. */
#define OFDMRX_FADING_SINES 16        /* sinusoids per path */
#define OFDMRX_FADING_KNOT 32         /* samples between two knots of a path's gain */
#define OFDMRX_FADING_MAX_DELAY 1024  /* samples */
typedef struct {
	int32_t ntaps;                                          /* 1..8 */
	int32_t delays[8];                                      /* samples */
	float gains_re[8], gains_im[8], spread_hz[8];
} ofdmrx_fading;
int ofdmrx_util_fading(ofdmrx_handle *h, const int16_t *d_in, size_t n_in,
	int16_t *d_out, size_t n_out, size_t samples_per_frame,
	const ofdmrx_fading *fd, uint64_t seed, uint64_t first_frame);

/* Wideband front end (added within revision 1.9, detected by symbol): one wideband I/Q capture at decim x the handle's rate ->
 * n_channels receiver channels at the handle's rate, each mixed down from its centre frequency, low-pass filtered and decimated.
 * DESIGN.md section 4.14 is the definition, held component by component to a float64 model:
 *   taps    K = 12 decim, T = 2 K + 1, h[k] = (0.75 / decim) sinc(0.75 (k - K) / decim) blackman(k, T), computed in double,
 *           normalised to sum 1, rounded once to fp32.  Flat within 0.01 dB up to rate / 4, below -70 dB from rate / 2 on.
 *   phase   inc_c = (uint32) llrint(centre_hz[c] 2^32 / (decim rate)); the phase at ABSOLUTE wideband index m is (inc_c m) mod 2^32
 *   output  y_c[n] = sum_k h[k] x[n decim - k] e^{-2 pi i phase_c(n decim - k) / 2^32}, x zero at negative indices; fp32 I/Q, no clip
 * Every output is a closed form of absolute indices: there is no state, and a capture cut into blocks (each block handed over with
 * the T - 1 samples before it) gives the same bytes as one call.  W samples give ceil(W / decim) outputs per channel.  Output n is
 * wideband time n decim - K: a signal appears 12 output samples late (ofdmrx_frame_result.sc_start lies 12 behind).
 * ofdmrx_util_channelize_taps: host only; writes the T taps, returns T; decim outside 2..32 or NULL taps: OFDMRX_E_ARG.
 * ofdmrx_util_channelize: DEVICE buffers, asynchronous on the handle's stream (a call with another decim or other centres than
 * the call before waits for the stream first); centre_hz is a HOST array.  d_in holds the wideband positions in_first .. in_first +
 * n_in - 1 as interleaved I/Q of sample_format (scaled as the decoder scales its input); output n (out_first .. out_first + n_out
 * - 1) of channel c lands at d_out + 2 (c out_stride + n - out_first) floats.  OFDMRX_E_ARG, before any device call and with the
 * output untouched: NULL pointers or zero counts; n_channels outside 1..65535; decim outside 2..32; a bad format; a negative in_first
 * or out_first; out_stride < n_out; a centre that is not finite or lies outside +- decim rate / 2; a position the outputs need that
 * is not in the buffer - in_first > 0 and out_first decim - (T - 1) < in_first, or (out_first + n_out - 1) decim > in_first + n_in -
 * 1 (with in_first == 0 the positions below 0 are zeros); d_out overlapping d_in; d_in off the sample-frame boundary, d_out off 8
 * bytes; positions or counts above 2^50; a handle with an open feed or bank. */
int ofdmrx_util_channelize_taps(int decim, float *taps);
int ofdmrx_util_channelize(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride);

/* Wideband front end at a rational decimation (added within revision 1.9, detected by symbol): a capture at Rw = rate p / q (formed
 * in double) for ANY ratio with 1 <= q <= 16 and 2 <= p / q <= 32 in lowest terms - the entries reduce by the gcd themselves, (50, 8)
 * is (25, 4).  DESIGN.md section 4.17 is the definition, held component by component to a float64 model.  With D = p / q, K = 12 D
 * (both real) and T = floor(24 p / q) + 1 taps per phase:
 *   time    u_n = n p (64 bits), i_n = u_n div q, q_n = u_n mod q: output n stands at wideband time i_n + q_n / q - K, 12 output
 *           samples late as above
 *   taps    g(t) = sinc(0.75 t / D) (0.42 + 0.5 cos(pi t / K) + 0.08 cos(2 pi t / K)) for |t| <= K, 0 outside;
 *           h_r[j] = g(j + r / q - K), j = 0 .. T - 1, r = 0 .. q - 1: in double, each phase normalised to sum 1, rounded once to
 *           fp32.  Every phase is flat within 0.01 dB up to rate / 4 and below -70 dB from rate / 2 on; the phases of one ratio
 *           differ from their mean by -100 dB or less in the pass band.
 *   phase   inc_c = (uint32) llrint(centre_hz[c] 2^32 / Rw); the phase at ABSOLUTE wideband index m is (inc_c m) mod 2^32
 *   output  y_c[n] = sum_j h_{q_n}[j] x[i_n - j] e^{-2 pi i phase_c(i_n - j) / 2^32}, x zero at negative indices; fp32 I/Q, no clip,
 *           summed with j ascending
 * No state: a capture cut into blocks (each handed over with the T - 1 samples before it) gives the same bytes as one call.  W
 * samples give ceil(W q / p) outputs per channel.
 * ofdmrx_util_channelize_ratio_taps: host only; writes [q][T] floats for the REDUCED ratio (at most 16 x 769), returns T.
 * ofdmrx_util_channelize_ratio: arguments, memory spaces, asynchrony and refusals are those of ofdmrx_util_channelize, with the
 * position test restated - refused if in_first > 0 and (out_first p div q) - (T - 1) < in_first, or ((out_first + n_out - 1) p div
 * q) > in_first + n_in - 1 - and centres outside +- Rw / 2 refused.  Both: OFDMRX_E_ARG, before any device call and with the output
 * untouched, for p or q <= 0, a reduced q above 16, p / q outside 2..32.  With reduced q = 1 both forward to the integer entries:
 * the same bytes by construction. */
int ofdmrx_util_channelize_ratio_taps(int p, int q, float *taps);
int ofdmrx_util_channelize_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride);

/* Wideband front end for a real capture (added within revision 1.9, detected by symbol): a ONE-channel capture - a sound-card
 * recording of a receiver's audio or IF, the real IF of a direct-sampling receiver - at Rw = rate p / q -> n_channels receiver
 * channels at the handle's rate.  For a real x the mix-down and low-pass is itself the Hilbert step: the stop band removes the mirror
 * image.  DESIGN.md section 4.25 is the definition, held component by component to a float64 model.  p / q is reduced by its gcd, with
 * the limits of ofdmrx_util_channelize_ratio (1 <= q <= 16, 2 <= p / q <= 32; q = 1 is the integer decimation D = p); Rw, K, T, the
 * taps (h at q = 1, else h_r[j]), the times i_n, q_n and the increment inc_c are those of ofdmrx_util_channelize and
 * ofdmrx_util_channelize_ratio, unchanged: there is no new filter.
 *   input   ONE value per wideband position, S16, U8 or F32, scaled as the decoder scales a mono sample; x zero at negative indices
 *   output  y_c[n] = 2 sum_j h_{q_n}[j] x[i_n - j] e^{-2 pi i phase_c(i_n - j) / 2^32}, fp32 I/Q, no clip.  The 2 makes a real cosine
 *           of amplitude A an analytic signal of amplitude A - what the mono decoder's own front end makes of it, and what the real
 *           part of a synthesized capture needs for a unity round trip.
 *   sums    those of ofdmrx_util_channelize (q = 1) or ofdmrx_util_channelize_ratio on the capture (x, +0) in the same order, with
 *           the products by the zero component left out - one FMA chain per component - and the multiplication by 2 last.  The
 *           output is, BYTE FOR BYTE, twice the output of those entries on the same samples with a +0 imaginary part.
 * No state: a capture cut into blocks (each handed over with the T - 1 samples before it) gives the same bytes as one call.
 * Centres: a real capture holds every signal at +f and its conjugate at -f, so the channel at centre f sees its mirror at distance
 * 2 |f| (mod Rw).  The pass band is flat to rate / 4 on either side, so a centre with |f| < rate / 4 or |f| > Rw / 2 - rate / 4, where
 * the mirror's pass band overlaps the channel's own, is refused.  From rate / 4 to about 0.35 rate (and as near Rw / 2) the mirror lies
 * in the filter's transition band: it comes out attenuated and outside the modem's own band, and is NOT refused - the reference's
 * default offset of 2000 Hz at 8 kHz is such a centre.  A negative centre is legal and gives the channel of the conjugate spectrum:
 * that is how the inverted audio of a lower-sideband receiver is decoded.
 * n_in counts samples and d_in must sit on the sample's boundary; every other argument, memory space, asynchrony and refusal is
 * ofdmrx_util_channelize_ratio's, with the centre rule above (and a centre that is not finite) in place of "outside +- Rw / 2".
 * OFDMRX_E_ARG comes before any device call and leaves the output untouched.  Not built: the real-input grid banks, the surveys of a
 * real capture, a synthesizer that writes one channel. */
int ofdmrx_util_channelize_real(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride);

/* Wideband front end on a channel grid (added within revision 1.9, detected by symbol): a polyphase filter bank for channels on a
 * raster.  DESIGN.md section 4.19 is the definition, held component by component to a float64 model.  With `rate` the handle's rate:
 *   D = decim, one of 2, 4, 8 .. 512; Rw = D rate; M = 2 D slots k = -M/2 .. M/2 - 1, slot k's centre at k rate / 2 (the slots lie
 *   half a channel rate apart: the bank is oversampled by 2); K = 12 D, T = 24 D + 1 = 12 M + 1
 *   taps    h[t]: the formula of ofdmrx_util_channelize_taps unchanged - in double, normalised to sum 1, rounded once to fp32; for
 *           D <= 32 the bytes that entry writes, for larger D the same filter scaled (flat within 0.01 dB up to rate / 4, -70 dB or
 *           below from rate / 2 on)
 *   output  y_k[n] = sum_{t = 0 .. T - 1} h[t] x[n D - t] e^{-2 pi i k (n D - t) / M}, x zero at negative indices; fp32 I/Q, no
 *           clip.  2^32 / M is an integer, so this is ofdmrx_util_channelize's output for the centre k rate / 2 with the increment
 *           k 2^32 / M and no rounding of it.  Group delay (12 output samples), sc_start + 12 and ceil(W / D) outputs per channel as
 *           there
 *   form    u_n[r] = sum_a h[r + M a] x[n D - r - M a], r = 0 .. M - 1, a = 0 .. 11 and a = 12 for r = 0: one fp32 fused
 *           multiply-add chain per component, a ascending, positions outside the buffer entering as +0;
 *           y_k[n] = (-1)^{k n} sum_r u_n[r] e^{+2 pi i k r / M}: an unnormalised inverse DFT of length M, whose order of
 *           operations is fixed by M alone.  No NCO
 * No state: a capture cut into blocks (each handed over with the T - 1 samples before it) gives the same bytes as one call.  The
 * outputs agree with ofdmrx_util_channelize at the same centres within the two tolerances, not byte for byte.
 * ofdmrx_util_channelize_grid_taps: host only; writes T floats (at most 12289), returns T; OFDMRX_E_ARG for a decim that is no power
 * of two in 2..512 or a NULL pointer.
 * ofdmrx_util_channelize_grid: row j of the output is slot slots[j] (a host array; NULL with n_slots = M: every slot in ascending k);
 * the other arguments, memory spaces, asynchrony and refusals are those of ofdmrx_util_channelize.  OFDMRX_E_ARG besides, before
 * any device call and with the output untouched: a decim that is no power of two in 2..512, a slot outside -M/2 .. M/2 - 1, n_slots
 * outside 1..65535, NULL slots with n_slots != M. */
int ofdmrx_util_channelize_grid_taps(int decim, float *taps);
int ofdmrx_util_channelize_grid(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	const int32_t *slots, size_t n_slots, long long out_first, size_t n_out, float *d_out, size_t out_stride);

/* Wideband front end on a channel grid at any ratio P / Q (added within revision 1.9, detected by symbol): the filter bank above for
 * the capture rates that are no power of two times the handle's rate.  DESIGN.md section 4.22 is the definition, held component by
 * component to a float64 model.  p / q is reduced by its gcd here; then 1 <= q <= 16, 2 q <= p <= 512 and p has no prime factor
 * other than 2, 3 and 5.  Rw = rate p / q, M = 2 p, T = 24 p div q + 1; the taps h_r[j] are ofdmrx_util_channelize_ratio_taps' (the
 * same formula beyond p / q = 32), the output times u_n = n p, i_n = u_n div q, q_n = u_n mod q those of ofdmrx_util_channelize_ratio.
 * Slot k lies at k rate / 2; the slots are the k with -p <= k q < p: k_first = -(p div q) .. ceil(p / q) - 1.
 *   output  y_k[n] = sum_{j = 0 .. T - 1} h_{q_n}[j] x[i_n - j] e^{-2 pi i (k q (i_n - j) mod M) / M}, x zero at negative indices;
 *           fp32 I/Q, no clip; the phase is integer arithmetic.  Group delay, sc_start + 12, the ceil(W q / p) outputs per channel
 *           and the positions a call needs are ofdmrx_util_channelize_ratio's
 *   form    u_n[r] = sum_a h_{q_n}[r + M a] x[i_n - r - M a] over the a with r + M a <= T - 1: one fp32 fused multiply-add chain
 *           per component, a ascending, positions outside the buffer entering as +0; a transform of length M from radix 5, 3, 4
 *           and 2 stages whose order is fixed by M alone; one complex multiply by the root of k q i_n mod M
 * No state: a capture cut into blocks (each handed over with the T - 1 samples before it) gives the same bytes as one call.  At q = 1
 * with p a power of two every entry below is the grid entry above at decim = p: its kernel, its bytes.
 * ofdmrx_util_channelize_grid_ratio_taps: host only; writes q rows of T floats, returns T.
 * ofdmrx_util_grid_ratio_slots: host only; the first slot and the number of slots.
 * ofdmrx_util_channelize_grid_ratio: row j of the output is slot slots[j] (a host array; NULL with n_slots = n_all: every slot in
 * ascending k); the other arguments, memory spaces, asynchrony and refusals are those of ofdmrx_util_channelize_ratio.
 * ofdmrx_bank_begin_wideband_grid_ratio: ofdmrx_bank_begin_wideband_grid at the ratio; push, end and the queries are the bank's.
 * OFDMRX_E_ARG besides, before any device call and with the output untouched: a ratio outside the above, a slot outside the range,
 * n_slots outside 1..65535, NULL slots with n_slots != n_all, a NULL pointer. */
int ofdmrx_util_channelize_grid_ratio_taps(int p, int q, float *taps);
int ofdmrx_util_grid_ratio_slots(int p, int q, int32_t *k_first, size_t *n_all);
int ofdmrx_util_channelize_grid_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const int32_t *slots, size_t n_slots, long long out_first, size_t n_out, float *d_out, size_t out_stride);
int ofdmrx_bank_begin_wideband_grid_ratio(ofdmrx_handle *h, size_t n_slots, const int32_t *slots, int p, int q, int sample_format);

/* Wideband synthesizer (added within revision 1.9, detected by symbol), the mirror image of the wideband front end: n_channels
 * narrowband transmissions at the handle's rate - what the device transmitter and the channel kernels leave - are each placed at a
 * centre frequency, a start time and a gain and summed into ONE wideband I/Q capture at interp x the handle's rate.  DESIGN.md
 * section 4.15 is the definition, held component by component to a float64 model.  With D = interp, Rw = D rate, K = 12 D, T = 24 D
 * + 1 and h[k] the fp32 taps ofdmrx_util_channelize_taps(D, .) writes - there is no new filter:
 *   input   x_c[j], j = 0 .. n_in - 1: sample frame c in_stride + j of d_in, interleaved I/Q of in_format (S16 or F32, scaled as the
 *           decoder scales its input); zero outside
 *   phase   inc_c = (uint32) llrint(centre_hz[c] 2^32 / Rw); the phase at ABSOLUTE wideband index m is (inc_c m) mod 2^32 - the
 *           expression of the front end, so a channel synthesized and channelized at one centre has no residual frequency at all
 *   gain    G_c = D gain[c], formed in double, rounded once to fp32 (the D restores what zero-stuffing removes)
 *   output  w[m] = sum_c G_c e^{+2 pi i phase_c(m) / 2^32} sum_j h[m - start[c] - j D] x_c[j], over the j with 0 <= m - start[c] -
 *           j D <= T - 1; start[c] >= 0 in wideband samples, need not be a multiple of D.  F32 output: (re, im) of w[m], no clip, a zero always +0.
 *           S16 output: the F32 output through the channel kernels' quantiser, nearbyintf(32767 clamp(v, -1, 1)): never -32768.
 * Every output is a closed form of absolute indices: there is no state, and a capture made window by window has the bytes of one
 * made in one call.  Sample j of channel c sits at wideband time start[c] + j D + K; through ofdmrx_util_channelize at the same
 * centre and D it comes out at index j + 24 + start[c] / D - exactly where D divides start[c], by a fractional delay otherwise.
 * The filter is flat to rate / 4 and down by 75 dB from rate / 2 on: make a 2-channel transmission for it with freq_off = 0 (its
 * band is at most +-1600 Hz at 8 kHz).  One at the default +2000 Hz reaches into the transition band and comes out attenuated; it
 * is not refused.
 * DEVICE buffers d_in and d_out, HOST arrays centre_hz, start and gain; asynchronous on the handle's stream.  Calls with other
 * parameter arrays than the call before take the next of a small ring of parameter sets and wait only for the launch that used
 * that set four changes ago.  Output m (out_first .. out_first + n_out - 1) lands m - out_first sample frames into d_out.
 * OFDMRX_E_ARG, before any device call and with the output untouched: NULL pointers or zero counts; n_channels outside 1..65535;
 * interp outside 2..32; an in_format or out_format other than S16 or F32; in_stride < n_in; a negative out_first or start; a centre
 * that is not finite or lies outside +- Rw / 2; a gain that is not finite (or so large that D gain is not); positions or counts
 * above 2^50 (n_out above 2^41 - 1024, which the launch cannot hold; in_stride above 2^34); d_out overlapping d_in; d_in or d_out
 * off its sample-frame boundary; a handle with an open feed or bank. */
int ofdmrx_util_synthesize(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int interp,
	const double *centre_hz, const long long *start, const float *gain, size_t n_channels, long long out_first, size_t n_out,
	void *d_out, int out_format);

/* Wideband synthesizer at a rational interpolation (added within revision 1.9, detected by symbol), the mirror image of the front end
 * at a rational decimation: a capture at Rw = rate p / q (formed in double) for ANY ratio with 1 <= q <= 16 and 2 <= p / q <= 32 in
 * lowest terms - the entry reduces by the gcd itself, (50, 8) is (25, 4).  DESIGN.md section 4.18 is the definition, held component
 * by component to a float64 model.  With D = p / q and K = 12 D (both real) and H[r][j] the fp32 table [q][T], T = floor(24 p / q) +
 * 1, that ofdmrx_util_channelize_ratio_taps(p, q, .) writes - there is no new filter - read as one sequence on the grid of 1 / q
 * wideband samples, G[tn] = H[tn mod q][tn div q], tn = 0 .. 24 p:
 *   input, phase: as ofdmrx_util_synthesize, with this Rw
 *   gain    G_c = D gain[c], D = (double)p / (double)q, formed in double, rounded once to fp32
 *   output  at ABSOLUTE wideband index m, r = m - start[c] (nothing where r < 0), nu = r q (64 bits), q0 = nu div p, b = nu mod p:
 *           w[m] = sum_c G_c e^{+2 pi i phase_c(m) / 2^32} sum_a G[b + a p] x_c[q0 - a], a = 0 .. 23, and a = 24 where b = 0.  F32 and
 *           S16 output as ofdmrx_util_synthesize writes them: a zero always +0, never -32768.
 * A channel's support is start[c] .. start[c] + ((n_in - 1 + 24) p) div q.  No state: a capture made window by window has the bytes
 * of one made in one call.  Sample j of channel c sits at wideband time start[c] + j D + K; through ofdmrx_util_channelize_ratio at
 * the same centre and ratio it comes out at index j + 24 + start[c] q / p - exactly where p divides start[c], by a fractional delay
 * otherwise.
 * Arguments, memory spaces, asynchrony, the ring of parameter sets (a set belongs to its ratio: 25/4 after 6, or after 25/3, never
 * reuses one) and every refusal are those of ofdmrx_util_synthesize, with the ratio's limits in place of interp's: OFDMRX_E_ARG,
 * before any device call and with the output untouched, for p or q <= 0, a reduced q above 16, p / q outside 2..32; a centre outside
 * +- Rw / 2; a gain for which D gain is not finite; n_out above 2^41 - 1024, which the launch cannot hold.  With reduced q = 1 it
 * forwards to ofdmrx_util_synthesize: the same bytes by construction. */
int ofdmrx_util_synthesize_ratio(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const double *centre_hz, const long long *start, const float *gain, size_t n_channels, long long out_first, size_t n_out,
	void *d_out, int out_format);

/* Wideband synthesizer on a channel grid (added within revision 1.9, detected by symbol), the mirror image of the front end on a
 * channel grid: a polyphase synthesis bank for rows on the raster rate / 2, interp a power of two 2 .. 512.  DESIGN.md section 4.20
 * is the definition, held component by component to a float64 model.  With D = interp, M = 2 D, T = 24 D + 1 and h[k] the fp32 taps
 * ofdmrx_util_channelize_grid_taps(D, .) writes - there is no new filter - row c belongs to slot k_c = slots[c] in -M/2 .. M/2 - 1
 * (a host array of pairwise distinct slots; NULL with n_slots = M: every slot in ascending k), with its centre at k_c rate / 2:
 *   output  w[m] = sum_c G_c e^{+2 pi i k_c m / M} sum_j h[m - start[c] - j D] x_c[j], over the j with 0 <= m - start[c] - j D <=
 *           T - 1; G_c = D gain[c] as in ofdmrx_util_synthesize; start[c] >= 0 in wideband samples, a MULTIPLE OF D.
 * This is ofdmrx_util_synthesize's output for the centres k_c rate / 2 (within the two tolerances: the sums are formed in another
 * order), at a cost per output that does not grow with the number of rows: one M-point transform per input time shared by all
 * slots, one pass of the filter, no NCO.  F32 and S16 output as ofdmrx_util_synthesize writes them: a zero always +0, never
 * -32768.  No state: a capture made window by window has the bytes of one made in one call.  Through ofdmrx_util_channelize_grid
 * at the same D and slot, sample j of row c comes out at index j + 24 + start[c] / D, exactly.
 * Arguments, memory spaces, asynchrony and the ring of parameter sets (a grid set is never taken for a plain one at the same D, nor
 * the reverse) are ofdmrx_util_synthesize's.  The handle keeps a scratch buffer of at most 32 MiB and cuts a call into chunks of
 * ofdmrx_util_synthesize_grid_chunk(interp) outputs, counted from out_first rounded down to a multiple of D; a seam changes no byte.
 * OFDMRX_E_ARG, before any device call and with the output untouched: everything ofdmrx_util_synthesize refuses except its range of
 * interp; an interp that is no power of two in 2 .. 512; a slot outside -M/2 .. M/2 - 1 or given twice; n_slots outside 1 .. M;
 * NULL slots with n_slots != M; a start that interp does not divide.
 * ofdmrx_util_synthesize_grid_chunk: host only; the outputs per chunk (a multiple of D), OFDMRX_E_ARG for such an interp. */
int ofdmrx_util_synthesize_grid(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int interp,
	const int32_t *slots, const long long *start, const float *gain, size_t n_slots, long long out_first, size_t n_out,
	void *d_out, int out_format);
long long ofdmrx_util_synthesize_grid_chunk(int interp);

/* Wideband synthesizer on a channel grid at any ratio P / Q (added within revision 1.9, detected by symbol), the mirror image of
 * ofdmrx_util_channelize_grid_ratio: a mixed-radix synthesis bank.  DESIGN.md section 4.23 is the definition, held component by
 * component to a float64 model.  p / q is reduced here; in lowest terms 1 <= q <= 16, 2 q <= p <= 512, p = 2^a 3^b 5^c - the limits of
 * ofdmrx_util_channelize_grid_ratio.  The capture's rate is rate p / q, M = 2 p, and G[tn], tn = 0 .. 24 p, is the tap sequence of
 * ofdmrx_util_synthesize_ratio (G[tn] = H[tn mod q][tn div q] over the table ofdmrx_util_channelize_grid_ratio_taps(p, q, .) writes;
 * there is no new filter).  Row c belongs to slot k_c = slots[c] with -p <= k_c q < p (a host array of pairwise distinct slots; NULL
 * with n_slots = n_all of ofdmrx_util_grid_ratio_slots: every slot in ascending k), centred at k_c rate / 2.  With m q = J p + beta
 * (0 <= beta < p) at the absolute wideband index m:
 *   output  w[m] = sum_c G_c e^{+2 pi i (k_c q m mod M) / M} sum_a G[beta + a p] x_c[J - a - start[c] q / p], a = 0 .. 23, and a = 24
 *           where beta = 0; G_c = (p / q) gain[c] as in ofdmrx_util_synthesize_ratio; start[c] >= 0 in wideband samples, a MULTIPLE
 *           OF p.
 * This is ofdmrx_util_synthesize_ratio's output for the centres k_c rate / 2 (within the two tolerances and that entry's rounding of
 * the phase increment), at a cost per output that does not grow with the number of rows, and it reaches p / q up to 512.  F32 and
 * S16 output as ofdmrx_util_synthesize writes them: a zero always +0, never -32768.  No state: a capture made window by window has
 * the bytes of one made in one call.  Through ofdmrx_util_channelize_grid_ratio at the same ratio and slot, sample j of row c comes
 * out at index j + 24 + start[c] q / p.  With reduced q = 1 and p a power of two it is ofdmrx_util_synthesize_grid: the same bytes.
 * Arguments, memory spaces, asynchrony and the ring of parameter sets (a ratio-grid set is never taken for a grid set or a plain one
 * at the same p / q) are ofdmrx_util_synthesize_grid's.  The handle's scratch of at most 32 MiB holds 2 q complex values per output;
 * a call is cut into chunks of ofdmrx_util_synthesize_grid_ratio_chunk(p, q) outputs, counted from out_first rounded down to a
 * multiple of p; a seam changes no byte.
 * OFDMRX_E_ARG, before any device call and with the output untouched: everything ofdmrx_util_synthesize_grid refuses except its rule
 * that interp is a power of two; a ratio ofdmrx_util_channelize_grid_ratio refuses; a slot outside -p <= k q < p or given twice;
 * n_slots outside 1 .. n_all; NULL slots with n_slots != n_all; a start that p does not divide; n_out above 2^41 - 1024.
 * ofdmrx_util_synthesize_grid_ratio_chunk: host only; the outputs per chunk (a multiple of p), OFDMRX_E_ARG for such a ratio. */
int ofdmrx_util_synthesize_grid_ratio(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const int32_t *slots, const long long *start, const float *gain, size_t n_slots, long long out_first, size_t n_out,
	void *d_out, int out_format);
long long ofdmrx_util_synthesize_grid_ratio_chunk(int p, int q);

/* Wideband survey (added within revision 1.9, detected by symbol): which bands of a wideband capture are occupied - the centres to
 * open the front end or a wideband bank on.  DESIGN.md section 4.16 is the definition, held bin by bin to a float64 model.
 * ofdmrx_util_survey: an averaged (Welch) power spectrum, one row or a waterfall of rows.  With N = nfft (1280, 2560 or 5120),
 * H = N / 2, S = segs_per_row (1 .. 65536) and Rw the capture's rate:
 *   window  periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / N), computed in double, rounded once to fp32; U = sum w[n]^2 over the fp32 values
 *   segment s >= 0 covers the wideband positions s H .. s H + N - 1;  X_s[b] = sum_n w[n] x[s H + n] e^{-2 pi i b n / N}
 *   row r   P[r][i] = (1 / (S U)) sum_{s = r S .. r S + S - 1} |X_s[(i + N / 2) mod N]|^2,  i = 0 .. N - 1 in ASCENDING frequency:
 *           index i is the frequency (i - N / 2) Rw / N.  White noise of power sigma^2 per complex sample reads sigma^2 in every bin.
 * Every output is a closed form of absolute indices: there is no state, and a capture surveyed row by row, each call given only
 * the samples its rows need, gives the same bytes as one call (the fp32 sums run over groups of 8 consecutive segments counted from
 * the row's first, then over the groups, both ascending).
 * ofdmrx_util_survey_window: host only; writes the N window values, returns N; another N or NULL: OFDMRX_E_ARG.
 * ofdmrx_util_survey: DEVICE buffers, asynchronous on the handle's stream.  d_in holds the wideband positions in_first .. in_first +
 * n_in - 1 as interleaved I/Q of sample_format (scaled as the decoder scales its input); row r (row_first .. row_first + n_rows - 1)
 * lands at d_out + (r - row_first) N floats.  OFDMRX_E_ARG, before any device call and with the output untouched: NULL pointers or
 * zero counts; a bad format; N outside the set; S outside 1..65536; a negative in_first or row_first; a position the rows need that
 * is not in the buffer - there is no zero padding: row_first S H < in_first, or (row_first + n_rows) S H + H > in_first + n_in; d_in
 * off the sample-frame boundary, d_out off 4 bytes; d_out overlapping d_in; positions or counts above 2^50; n_rows ceil(S / 8) N
 * above 2^28 (the partial sums of one call: 1 GiB), which the launch cannot hold; a handle with an open feed or bank.
 * ofdmrx_util_find_bands: host only, float64; the bands of ONE row psd[0 .. N - 1] of a capture at rate_wide:
 *   floor     max(median of the N values, abs_floor); the median is the mean of the two middle values.  It is the noise floor only
 *             while less than half the band is occupied: give abs_floor where that may not hold.
 *   occupied  bin i with psd[i] > floor 10^(thr_db / 10) and psd[i] > 0
 *   run       occupied bins separated by at most floor(gap_hz / (rate_wide / N)) unoccupied bins; runs do not wrap round the band edge
 *   band      a run first .. last of width (last - first + 1) rate_wide / N >= min_width_hz (a DC spike or a carrier is dropped by
 *             this); centre_hz = ((first + last) / 2 - N / 2) rate_wide / N; power = mean of psd over first .. last; level_db = 10
 *             log10(power / floor)
 * Bands come in ascending frequency; *n_bands counts all of them, only the first max_bands are written; *floor_out (nullable) gets
 * the floor.  OFDMRX_E_ARG: NULL psd, bands or n_bands; N outside the set; rate_wide that is not finite or <= 0; thr_db, gap_hz,
 * min_width_hz or abs_floor that is not finite or negative. */
typedef struct ofdmrx_band {
	double centre_hz, width_hz, power;
	float level_db;
	int32_t first_bin, last_bin;
} ofdmrx_band;
int ofdmrx_util_survey_window(int nfft, float *w);
int ofdmrx_util_survey(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int nfft,
	int segs_per_row, long long row_first, size_t n_rows, float *d_out);
int ofdmrx_util_find_bands(const float *psd, int nfft, double rate_wide, double thr_db, double gap_hz, double min_width_hz,
	double abs_floor, size_t max_bands, ofdmrx_band *bands, size_t *n_bands, double *floor_out);

/* Grid survey (added within revision 1.9, detected by symbol): which slots of the channel grid hold a signal - the slots to open the
 * grid front end or a grid bank on.  DESIGN.md section 4.21 is the definition, held slot by slot to a float64 model.
 * ofdmrx_util_survey_grid: the mean output power of every slot of the grid front end's filter bank, one row or a waterfall of rows.
 * With D = decim (a power of two 2 .. 512), M = 2 D, the taps and y_k[n] of the grid front end above at ABSOLUTE output times n (the
 * capture zero at negative positions) and S = times_per_row, a multiple of 8 in 8 .. 65536:
 *   row r   P[r][k + M / 2] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2,  k = -M / 2 .. M / 2 - 1: ASCENDING slot order, index i
 *           is slot i - M / 2 at (i - M / 2) rate / 2.  No further normalisation: P is the mean power the slot's decoder sees, and
 *           white noise of power sigma^2 per complex sample reads sigma^2 sum h^2, about 0.7071 sigma^2 / D.
 * Row r needs the wideband positions max(0, (r S - 24) D) .. ((r + 1) S - 1) D.  Every output is a closed form of absolute indices:
 * there is no state, and a capture surveyed row by row, each call given only the positions its rows need, gives the same bytes as
 * one call (the fp32 sums run over groups of 8 consecutive output times, then over a row's groups, both ascending).
 * DEVICE buffers, asynchronous on the handle's stream.  d_in holds the wideband positions in_first .. in_first + n_in - 1 as
 * interleaved I/Q of sample_format; row r (row_first .. row_first + n_rows - 1) lands at d_out + (r - row_first) M floats.
 * OFDMRX_E_ARG, before any device call and with the output untouched: NULL pointers or zero counts; a bad format; decim outside the
 * set; S no multiple of 8 or outside 8 .. 65536; a negative in_first or row_first; a position the rows need that is not in the
 * buffer - there is no zero padding other than below position 0; d_in off the sample-frame boundary, d_out off 4 bytes; d_out
 * overlapping d_in; positions or counts above 2^50; n_rows (S / 8) M above 2^28 (the partial sums of one call: 1 GiB); a handle
 * with an open feed or bank.
 * ofdmrx_util_find_slots: host only, float64; the occupied slots of ONE row row[0 .. M - 1] at the handle rate `rate`:
 *   floor     abs_floor if that is > 0, else the median of the M values (the mean of the two middle values).  Unlike find_bands'
 *             floor it is NOT the larger of the two: a bank with a few strong frames has more than half its slots above the noise
 *             (every frame lights its two neighbours through the filter's transition band), and only a given floor brings it down.
 *   occupied  slot i with row[i] > floor 10^(thr_db / 10) and row[i] > 0
 *   shadowed  slot i with a cyclic neighbour j = i +- 1 mod M whose row[j] > row[i] 10^(sep_db / 10): an edge of the neighbour's
 *             signal.  The rule's blind spot: a real signal more than sep_db below a neighbouring slot's is not found.
 * The occupied, unshadowed slots come in ascending order; *n_slots counts all of them, only the first max_slots are written:
 * slot = i - M / 2, centre_hz = slot rate / 2, power = row[i], level_db = 10 log10(power / floor).  *floor_out (nullable) gets the
 * floor.  OFDMRX_E_ARG: NULL row, slots or n_slots; decim outside the set; a rate that is not finite or <= 0; thr_db, sep_db or
 * abs_floor that is not finite or negative. */
typedef struct ofdmrx_slot {
	int slot;
	double centre_hz, power;
	float level_db;
} ofdmrx_slot;
int ofdmrx_util_survey_grid(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	int times_per_row, long long row_first, size_t n_rows, float *d_out);
int ofdmrx_util_find_slots(const float *row, int decim, double rate, double thr_db, double sep_db, double abs_floor,
	size_t max_slots, ofdmrx_slot *slots, size_t *n_slots, double *floor_out);

/* Grid survey at any ratio P / Q (added within revision 1.9, detected by symbol): the survey above for the raster of the grid front
 * end at a ratio - a capture at 48, 50, 250 or 300 kHz searched for the slots to open.  DESIGN.md section 4.24 is the definition,
 * held slot by slot to a float64 model.  p / q is reduced inside; in lowest terms 1 <= q <= 16, 2 q <= p <= 512, p with no prime
 * factor other than 2, 3 and 5.  With M = 2 p, the taps, the output times i_n = (n p) div q, q_n = (n p) mod q, the slots k_first ..
 * k_first + n_all - 1 (ofdmrx_util_grid_ratio_slots) and y_k[n] of the grid front end at a ratio above at ABSOLUTE output times n (the
 * capture zero at negative positions), and S = times_per_row, a multiple of 8 in 8 .. 65536:
 *   row r   P[r][k - k_first] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2: n_all floats in ASCENDING slot order, index i is
 *           slot k_first + i at (k_first + i) rate / 2.  No further normalisation.
 * Row r needs the wideband positions max(0, (r S p) div q - 24 p div q) .. (((r + 1) S - 1) p) div q.  The summation order is the
 * grid survey's; there is no state, and a capture surveyed row by row, each call given only the positions its rows need, gives the
 * same bytes as one call.  At reduced q = 1 with p a power of two the call IS ofdmrx_util_survey_grid at decim = p: its kernel, its
 * bytes, rows of M = n_all values.  The table on the device is the ratio-grid table with every slot, under the front end's key: a
 * survey between two front-end calls on other slots leaves their bytes unchanged, and the reverse.
 * DEVICE buffers, asynchronous on the handle's stream; row r (row_first .. row_first + n_rows - 1) lands at d_out + (r - row_first)
 * n_all floats.
 * OFDMRX_E_ARG, before any device call and with the output untouched: NULL pointers or zero counts; a bad format; a ratio outside
 * the set; S no multiple of 8 or outside 8 .. 65536; a negative in_first or row_first; a position the rows need that is not in the
 * buffer - there is no zero padding other than below position 0; d_in off the sample-frame boundary, d_out off 4 bytes; d_out
 * overlapping d_in; positions or counts above 2^50; n_rows (S / 8) n_all above 2^28; a handle with an open feed or bank.
 * ofdmrx_util_find_slots_ratio: host only, float64; ofdmrx_util_find_slots on the n_all values of ONE row at the ratio p / q:
 *   floor     abs_floor if that is > 0, else the median of the n_all values (an odd count: the middle value; an even count: the mean
 *             of the two middle values)
 *   occupied, shadowed: as above, but the neighbours are cyclic only where the slots tile the circle, n_all q = M (q = 1 or 2);
 *             otherwise slot k_first and the last slot have one neighbour each - beyond them lies no whole slot.  With r = p mod q the
 *             ends leave a gap of 2 r - q bins of M where r > q / 2 and OVERLAP by q - 2 r bins where r < q / 2: at 25/4 slot 6 and
 *             slot -6 lie half a slot apart across the band edge and a signal in one reads in the other at nearly full strength.
 *   the ends seen twice: where the centres of the last and the first slot lie half a slot apart or less (0 < 4 r <= q: 25/4, 9/4)
 *             two signals cannot stand there side by side.  If both ends are occupied and unshadowed and lie within sep_db of each
 *             other they are one signal: the louder is reported (a tie: k_first).  Further apart than sep_db both are reported -
 *             neither shadows the other.  Ends that overlap by less (q < 4 r < 2 q, 10/3) are both reported.
 * slot = k_first + i, centre_hz = slot rate / 2.  At q = 1 with p a power of two it returns what ofdmrx_util_find_slots returns.
 * OFDMRX_E_ARG: NULL row, slots or n_slots; a ratio outside the set; a rate that is not finite or <= 0; thr_db, sep_db or abs_floor
 * that is not finite or negative.
 * Not built: pruning the transform to the 2 p / q slot bins; p beyond 512 or other primes; and, the rule's blind spot as above, a
 * signal more than sep_db below a neighbour is not found; at a ratio whose ends overlap by less than half a slot one signal there
 * may be reported in both ends. */
int ofdmrx_util_survey_grid_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	int times_per_row, long long row_first, size_t n_rows, float *d_out);
int ofdmrx_util_find_slots_ratio(const float *row, int p, int q, double rate, double thr_db, double sep_db, double abs_floor,
	size_t max_slots, ofdmrx_slot *slots, size_t *n_slots, double *floor_out);

/* ---- N2: the transmitter on the device (replaces Encoder<value,cmplx,rate>(pcm, inp, count=1, freq_off,
 * call_sign, oper_mode), encode.cc:271,424-436, for batches; rate = the handle's sample_rate).  d_payload:
 * n_frames x 5380 UNSCRAMBLED bytes (what main() reads from the input files, encode.cc:414); d_pcm: n_frames x
 * ofdmrx_frame_samples(rate, mode) x channels int16, exactly the body of the WAV
 * `encode OUT RATE 16 CHANNELS OFFSET MODE CALLSIGN file` writes.  DEVICE pointers.
 * ofdmrx_frame_samples: sample frames of that one-payload file = 2 x rate of silence (encode.cc:423,441) +
 * (rows + 5) symbols; ofdmrx_tx_frame_samples(mode) is the 8 kHz value. */
long ofdmrx_frame_samples(int sample_rate, int oper_mode);
long ofdmrx_tx_frame_samples(int oper_mode);
/* Streams of `count` payloads, as `encode OUT RATE BITS CHANNELS OFFSET MODE CALLSIGN file1 .. fileN` writes them
 * (encode.cc:288-313: pilot | count x (S&C, meta, pilot, rows) | zero symbol, `rate` samples of silence either side),
 * bits = 8 (unsigned, offset 128) or 16.  ofdmrx_stream_samples: sample frames of one such stream.
 * _device: n_streams x count x 5380 payload bytes in, n_streams x samples x channels PCM out, DEVICE pointers;
 * asynchronous on the handle's stream like the decode entry (scratch is kept in the handle: no allocation per call).
 * ofdmrx_tx_encode_stream: the same for ONE stream with HOST pointers (what the `encode` CLI calls).
 * Arguments main() refuses are refused here with OFDMRX_E_ARG and nothing is written: a mode outside 6..13 (encode.cc:353), a call
 * sign outside 0 < value < 129961739795077 (encode.cc:358), a freq_off that is no multiple of 50 (encode.cc:394) or, since 1.9, one
 * that puts part of the band outside the spectrum (encode.cc:389, with band_width of encode.cc:363-387 and rate = the handle's):
 * freq_off < band_width / 2 - rate / 2, freq_off > rate / 2 - band_width / 2, or with one channel freq_off < band_width / 2. */
long ofdmrx_stream_samples(int sample_rate, int oper_mode, int count);
/* call sign -> the base-37 integer of the header (encode.cc:320-335: ' ' = 0, digits 1..10, letters of either case
 * 11..36), -1 if the string holds any other character.  Valid call signs are 0 < value < 129961739795077
 * (encode.cc:358, decode.cc:439). */
long long ofdmrx_callsign_value(const char *call_sign);
int ofdmrx_tx_encode_stream_device(ofdmrx_handle *h, const uint8_t *d_payload, size_t n_streams, int count,
	int oper_mode, int freq_off, const char *call_sign, int channels, int bits, void *d_pcm);
int ofdmrx_tx_encode_stream(ofdmrx_handle *h, const uint8_t *payload, int count, int oper_mode, int freq_off,
	const char *call_sign, int channels, int bits, void *pcm);
int ofdmrx_tx_encode_device(ofdmrx_handle *h, const uint8_t *d_payload, size_t n_frames, int oper_mode,
	int freq_off, const char *call_sign, int channels, int16_t *d_pcm);

#ifdef __cplusplus
}
#endif
#endif
