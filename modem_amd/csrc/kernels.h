// kernels.h -- structs shared by the host API (api_*.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_common.h"

namespace rx {

// one decode call's view of the raw PCM batch (what DSP::ReadPCM delivers, decode.cc:297-298)
struct FrameBatch {
	const void *samples;           // device pointer, frame 0
	size_t frame_stride_bytes;
	long samples_per_frame;
	int fmt;                       // OFDMRX_FMT_*
	int channels;                  // 1 or 2
};

// Many recordings in one call (ofdmrx_decode_streams): source q is src_len[q] sample frames at samples +
// q * frame_stride_bytes, and frame f of a launch reads source src_of[f] (src_of = nullptr: source f).  A kernel template takes
// either kind of batch: with a FrameBatch the two helpers below are what the kernels have always computed.
struct SourceBatch : FrameBatch {
	const int *src_of;             // [frames of the launch], nullable
	const int *src_len;            // [sources]
	const long long *tile0;        // the stream scan: [sources + 1] first tile of every source in the per-tile arrays (a running sum)
	const long long *given0;       // ofdmrx_debug_streams_edges: [sources] where its sequence starts in the packed timing values
};
// Live channels in one push (ofdmrx_bank_*, and ofdmrx_feed_* as a bank of one): channel q is a WINDOW of its stream.  Position 0 of channel q would
// lie at samples + org[q] (bytes; the channel's place in the slab minus its window's base, so it may be negative), the channel has
// been fed len[q] sample frames and its window holds the positions from lo[q] on.  The scan of a push takes the tiles tile0[q] ..
// of channel q, tile_at[q + 1] - tile_at[q] of them, at tile_at[q] in the per-tile arrays.  Frame f of a record launch reads
// channel src_of[f].  Positions are 64-bit throughout.
struct WindowBatch : FrameBatch {
	const int *src_of;             // [frames of the launch], nullable
	const long long *org;          // [channels]
	const long long *len;          // [channels]
	const long long *lo;           // [channels]
	const long long *tile0;        // [channels]
	const long long *tile_at;      // [channels + 1]
	long long *below;              // [channels] k_stream_accept: set when an edge of the channel would read below lo[q]
	// mono input: the analytic signal and the DC blocker's kept states, as org for the raw samples (bytes from z / ck of the launch);
	// dc_from: the DC blocker resumes at that position (a multiple of MONO_CK), fe0: first stretch the front end forms, fe_at: running sum
	const long long *z_org, *ck_org, *dc_from, *dc_at, *fe0, *fe_at;
};
__host__ __device__ inline int batch_source(const FrameBatch &, int f) { return f; }
__host__ __device__ inline long batch_len(const FrameBatch &fb, int) { return fb.samples_per_frame; }
__host__ __device__ inline int batch_source(const SourceBatch &fb, int f) { return fb.src_of ? fb.src_of[f] : f; }
__host__ __device__ inline long batch_len(const SourceBatch &fb, int q) { return fb.src_len[q]; }
__host__ __device__ inline int batch_source(const WindowBatch &fb, int f) { return fb.src_of ? fb.src_of[f] : f; }
__host__ __device__ inline long batch_len(const WindowBatch &fb, int q) { return (long)fb.len[q]; }
// where source q's position 0 lies
__host__ __device__ inline const char *batch_base(const FrameBatch &fb, int q) { return (const char *)fb.samples + (size_t)q * fb.frame_stride_bytes; }
__host__ __device__ inline const char *batch_base(const WindowBatch &fb, int q) { return (const char *)fb.samples + fb.org[q]; }

struct FrontCoef {                 // BlockDC::samples(2*(symbol_len+guard_len)) + Hilbert<cmplx,filter_len> (decode.cc:386,193)
	float dc_a, dc_b;
	float reco, imco[32];          // (filter_len-1)/4 odd-tap pairs: 5 / 10 / 28 / 31 at 8 / 16 / 44.1 / 48 kHz
};

// Mono input (round 4, mono_front.h): the DC blocker's one-pole low pass s[n] = a s[n-1] + g x[n] (y[n] = b x[n] - s[n-1]) with the
// powers of a its blocked scans use, computed once on the host in double, and the Hilbert taps.  ck: the state after every 64th
// sample of every frame (k_mono_carries).
struct MonoArgs {
	const double *ck;              // [n][ck_per_frame]
	int ck_per_frame;
	float a, g, b;
	float apw[8];                  // a^1 .. a^8
	float astep8[6], astep5[6];    // a^(8 2^k), a^(5 2^k): weights of the wave scans over thread chunks of 8 (MonoCover) / 5 (k_demod) samples
	double awave8, awave5;         // a^512, a^320: what a whole wave of such chunks decays by
	FrontCoef co;
};
inline MonoArgs mono_args(const FrontCoef &co, const double *ck, int ck_per_frame)
{
	MonoArgs m;
	m.ck = ck;
	m.ck_per_frame = ck_per_frame;
	const double a = (double)co.dc_a, b = (double)co.dc_b;
	m.a = (float)a; m.b = (float)b; m.g = (float)(b * (1.0 - a));
	double p = a;
	for (int i = 0; i < 8; ++i, p *= a)
		m.apw[i] = (float)p;
	double s8 = 1.0, s5 = 1.0;
	for (int i = 0; i < 8; ++i) s8 *= a;
	for (int i = 0; i < 5; ++i) s5 *= a;
	for (int k = 0; k < 6; ++k) {
		m.astep8[k] = (float)s8; m.astep5[k] = (float)s5;
		s8 *= s8; s5 *= s5;
	}
	m.awave8 = s8; m.awave5 = s5;
	m.co = co;
	return m;
}
inline int mono_ck_per_frame(long samples_per_frame) { return (int)((samples_per_frame + 63) / 64); }
// 8 kHz: the consumers form the analytic signal (launch_sync / _header / _demod with channels = 1).  The other rates (Hilbert filters of
// 41 - 125 taps, symbols of 2560 - 7680 samples) run launch_front_end over the whole stream first and read z like 2-channel input.
inline bool mono_fused(int rate) { return rate == 8000; }

struct SyncState {                 // per frame, across sync rounds (decode.cc:390-448 loop)
	long t_next;                   // next sample time to examine
	long sc_start;                 // stream index of the S&C body
	int active;                    // still searching in this round
	int found;                     // a preamble was accepted in THIS round.  Invariant across kernels: only launch_init_sync and k_header clear
	                               // it (k_header whenever it leaves active = 1 for another round, decode.cc:448), so the scan kernels of a
	                               // round may return early on it; a frame with active = 0 is never looked at again
	int symbol_pos;                // window coordinate, decode.cc:400
	float cfo_rad;
	int rejects;
	int skip_left;                 // decode.cc:448 while (skip_count--)
	int status;                    // OFDMRX_* so far
	int oper_mode;
	unsigned long long call_sign;
	int hdr_rounds;                // header attempts so far
	int okay;
	// a trigger found by the scanning kernel and not yet examined by the accept kernel (rates above 8 kHz, k_sync.hip)
	long pend_g;
	int pend_index_max;
	float pend_phase;
	int pending;
};

struct Tables {                    // device-resident constants, built once per handle
	const cf *tw_sym;              // e^{-j 2 pi m / symbol_len} (1280 at 8 kHz)
	const cf *sc_kern;             // conj(FFT(mls0))/(symbol_len/2), decode.cc:80-82
	const float *mls1_nrz;         // +-1 descrambler, decode.cc:407-409
	const float *mls0_nrz;         // [127] MLS 0b10001001 (transmitter: Schmidl-Cox symbol, encode.cc:144)
	const float *mls2_nrz;         // [512] MLS 0b100101010001 (transmitter: pilot block, encode.cc:134)
	const cf *tw_sym4;             // e^{-j 2 pi m / (4 symbol_len)} (transmitter PAPR step)
	const cf *tw_symc;             // compact per-stage twiddles of the symbol_len-point plan (transmitter: read through L1)
	const uint32_t *frozen;        // [2][2048] words, bit set = frozen: frozen_64800_43072, frozen_64512_43072 (regenerated)
	const uint16_t *info_pos;      // [2][44096] ascending unfrozen positions per table
	const uint32_t *info_compress; // [2][2048][8] per code word: compress move masks, unfrozen mask, first message bit | count << 16 (message_gather)
	const uint8_t *node_lev64;     // [2][1024] the same per 64-leaf block, for k_sc (frozen: 64 or 128 leaves, information: 64 .. 2048)
	const uint32_t *frozen_t;      // [2][16][64][2] frozen bits of a 4096-leaf sub-tree as lane `lane` of k_sc<6> holds it (bit x = leaf s * 4096 + x * 64 + position)
	const uint8_t *node_lev32;     // [2][2048] ... per 32-leaf block (frozen: 32 .. 128 leaves, information: 32 .. 1024)
	const uint8_t *node_lev;       // [2][8192] per 8-leaf group: level of the largest aligned all-frozen (low nibble) /
	                               // all-information (high nibble) node that starts there (frozen: <= 128 leaves, information: <= 2048), 0 = none
	const uint32_t *genmat_bits;   // BCH(255,71) systematic generator, [71][8] words, bit i of row j
	const uint8_t *osd_pairs;      // [2485][2] (a,b)
	const uint8_t *osd_triples;    // [57155][3] (a,b,c) sorted by c (equal d-loop lengths are adjacent)
	const uint32_t *crc32_tab;     // 256-entry byte table of CRC<uint32_t>(0xD419CC15)
	const uint32_t *crc32_shift168; // [4][256]: the CRC state advanced by 168 zero bytes, per state byte (k_finish)
	const uint32_t *crc32_adv;     // [256][32]: bit b of a state advanced by what follows segment k of the 5384 message bytes (crc32_wg256)
	const uint8_t *scramble;       // 5380 bytes of the Xorshift32 stream (decode.cc:613-615)
};

// ---- the list decoder's work queue (round 4).  Frames the syndrome certificate cannot finish are queued by k_back with their
// LLRs - entry e in slot e % cap of the slot arrays (LLRs, partial sums, metrics, ListSlot) - and k_polar / k_finish take
// whole runs of entries: a flush (api_pipeline.cpp) is k_queue_plan | k_polar | k_finish, and it takes nothing until one full
// residency of the list decoder waits, so a few stragglers per chunk no longer cost a decoder round each.  All counters live
// on the device: the host never waits to learn how many frames a chunk left.
struct ListQueue {
	unsigned tail;                 // entries allocated since the call began (k_back: atomicAdd)
	unsigned head;                 // entries taken by the flushes planned so far
	unsigned snap[2];              // tail behind k_back of the chunk with parity 0 / 1 (k_queue_snap): what that chunk's flush may take
	unsigned run_head[2], run_n[2];   // the entries of the flush of the chunk with parity 0 / 1 (k_queue_plan)
	int next_unit[2];              // k_polar's shared work counter, per flush
	int cert_on;                   // adaptive certificate: tried for every frame (1) or for a probe sample (0)
	unsigned tried, certified;     // since the last snapshot: frames the certificate was tried for / that it finished
	unsigned cap;                  // slots
	unsigned done_total;           // SC ring only: frames k_sc_finish has finished since the call began
	unsigned epoch;                // SC ring only: chunks since the call began (k_sc_adapt): the probe sample runs in every fourth
	unsigned probe_tried, probe_done;   // while cert_on = 0: the probe sample's counts, summed over chunks until eight frames have been tried
};
// The SC ring (k_sc.hip) is a second queue of the same shape in front of this one: k_back puts a frame there when the SC pass is
// on (its cert_on; tried / certified count the last run's entries / decided frames), k_sc_plan | k_sc | k_sc_finish run right behind
// k_back of every chunk on the same stream, and what they cannot decide moves on to the list decoder's queue.  Like a flush of the
// list decoder, a run takes WHOLE residencies of k_sc's persistent decoders (round 6: a codeword is one decoder's serial work of
// 1.2 ms, so a run of 8192 entries on the 2560 decoders of that time took four rounds for 3.2 rounds of work; 2048 decoders since the
// clean-node tests, k_sc.hip SC6_WAVES); what is left over waits
// for the next chunk's run, and the last run of a call takes everything.
struct ScStat { float metric, min_fork; int32_t ok, pad; };   // per SC-ring slot: P*'s metric, min_fork, rule holds
struct ListSlot {                  // what k_polar / k_finish need to know about a queued frame
	uint8_t *payload;              // where its 5380 bytes go when the list decoder's flush delivers them (k_finish)
	struct Result *res;            // its record (complete but for best_lane / bit_flips / a payload CRC failure)
	uint8_t *payload_now;          // the same in the chunk's own arrays: where k_sc_finish delivers, which runs right behind k_back -
	struct Result *res_now;        // before a staging buffer of the chunk leaves (launch_back: payload_later)
	int oper_mode;
	int frame;                     // index in its chunk
	int chunk;                     // which chunk of its call: a frame the list-1 pass finishes in a LATER chunk's run goes to payload / res
	int pad;
};
struct ScRing { ListQueue *q; ListSlot *slots; float *llr; };  // what k_back needs of the SC ring (q = nullptr: the pass is off)

struct Result {                    // device mirror of ofdmrx_frame_result (same layout)
	int32_t status;
	int32_t symbol_pos;
	int64_t sc_start;
	float cfo_rad, cfo_fine, sfo_slope;
	int32_t oper_mode;
	uint64_t call_sign;
	int32_t best_lane, bit_flips;
	float esn0_db_last;
	int32_t n_sync_rejects;
};

struct Attempt {                   // device mirror of ofdmrx_attempt: one preamble of a frame's SKIP loop (decode.cc:390-448)
	int32_t status, symbol_pos;
	float cfo_rad;
	int32_t oper_mode;
	uint64_t call_sign;
};
constexpr int ATTEMPTS_MAX = 65;   // OFDMRX_MAX_SKIP + 1

// ---- launch wrappers (defined next to their kernels) ------------------------
// `rate` selects the RateCfg instantiation (8000 / 16000 / 44100 / 48000)
// D1 (mono input, mono_front.h): ck = [n][mono_ck_per_frame()] states of the DC blocker; with mono_fused(rate) the consumers below
// form the analytic signal where they read it (ma.ck = ck) and z ([n][samples_per_frame]) is scratch the sync / header kernels
// write the windows they read into; launch_front_end fills all of z (the other rates; the ANALYTIC tap).  2-channel input: z, ma unused.
void launch_mono_carries(hipStream_t s, int rate, int n, FrameBatch fb, FrontCoef co, double *ck);
void launch_front_end(hipStream_t s, int rate, int n, FrameBatch fb, MonoArgs ma, cf *z);
void launch_sync(hipStream_t s, int rate, int n, FrameBatch fb, cf *z, Tables tb, SyncState *st, cf *scratch, const MonoArgs &ma);
// attempts / attempt_counts (nullable): [n][ATTEMPTS_MAX] records of the preambles examined so far, [n] their number
void launch_header(hipStream_t s, int rate, int n, FrameBatch fb, cf *z, const MonoArgs &ma, Tables tb, SyncState *st, int8_t *hdr_soft,
	Attempt *attempts = nullptr, int32_t *attempt_counts = nullptr);
void launch_osd_only(hipStream_t s, int n, Tables tb, const int8_t *soft, uint8_t *hard, int32_t *unique);
bool demod_forms_cons(int rate);   // cons is complete after k_demod (else k_theil_sen forms the rows from the carriers)
void launch_demod(hipStream_t s, int rate, int n, FrameBatch fb, cf *z, const MonoArgs &ma, Tables tb, const SyncState *st, cf *cons, cf *carr);
// the same two for records of many recordings (2-channel sources: mono input has been through launch_streams_front)
void launch_header_sources(hipStream_t s, int rate, int n, SourceBatch fb, Tables tb, SyncState *st, int8_t *hdr_soft);
void launch_demod_sources(hipStream_t s, int rate, int n, SourceBatch fb, Tables tb, const SyncState *st, cf *cons, cf *carr);
// ... and of many live channels (ofdmrx_bank_*): record f reads channel fb.src_of[f]'s window at its 64-bit absolute sc_start
void launch_header_bank(hipStream_t s, int rate, int n, WindowBatch fb, Tables tb, SyncState *st, int8_t *hdr_soft);
void launch_demod_bank(hipStream_t s, int rate, int n, WindowBatch fb, Tables tb, const SyncState *st, cf *cons, cf *carr);
void launch_theil_sen(hipStream_t s, int n, const SyncState *st, cf *cons, const cf *carr, float *slope, float *yint, int *chunk_flags);
void launch_theil_sen_raw(hipStream_t s, int rows, int cols, const float *y, float *slope, float *yint);
// D5's rotation + D6-D8 + the syndrome certificate (k_finish.hip: k_back).  cert_mode 0: every frame with a header goes to the list
// decoder's queue; 1: the certificate is tried (adaptively) and finishes the frames it decides (payload + result).
// esn0_rows (nullable): [n][ROWS_MAX] dB values, decode.cc:517-519; slot_of: [n] queue slot per frame, -1 = none.
// payload_later / res_later (nullable: payload / res): where k_finish delivers the frames this chunk leaves to the queue - the
// chunk's own arrays may be a staging buffer that has been copied out and reused by the time their flush comes
void launch_back(hipStream_t s, int rate, int n, int cert_mode, const SyncState *st, const cf *cons, const float *slope, const float *yint,
	float *precision, Result *res, float *esn0_rows, Tables tb, int descramble, uint8_t *payload, ListQueue *q, ListSlot *slots,
	float *llr_q, int *slot_of, uint8_t *payload_later = nullptr, Result *res_later = nullptr, ScRing sc = ScRing{ nullptr, nullptr, nullptr }, int chunk_seq = 0);
void launch_rotate_tap(hipStream_t s, const SyncState *st, const cf *cons, const float *slope, const float *yint, cf *out);   // one frame, CONS_MAX points
void launch_queue_reset(hipStream_t s, ListQueue *q, unsigned cap);
void launch_queue_snap(hipStream_t s, ListQueue *q, int par);
void launch_queue_plan(hipStream_t s, ListQueue *q, int par, unsigned unit, int force);
void launch_queue_fill(hipStream_t s, ListQueue *q, ListSlot *slots, int n, uint8_t *payload, Result *res, int oper_mode);
// the sign-following path alone + its certificate (k_sc.hip): grid = resident decoders (sc_store_bytes() of level store each),
// lb = log2 of the lanes per codeword: 5 (two codewords per wave), 6 (one), 0: both launched, the run's length picks one on the device
// unit: a run takes whole multiples of it (0 / force: everything that waits)
void launch_sc_plan(hipStream_t s, ListQueue *qs, unsigned unit = 0, int force = 1);
void launch_sc(hipStream_t s, int lb, int grid5, int grid6, ListQueue *qs, const ListSlot *slots, const float *llr_q, float *soft, unsigned long long *cw_q,
	unsigned long long *xw_q, ScStat *stat_q, Tables tb, int top_skip = 1);
void launch_sc_finish(hipStream_t s, int max_entries, ListQueue *qs, const ListSlot *slots_s, const float *llr_s, const unsigned long long *cw_q,
	const unsigned long long *xw_q, const ScStat *stat_q, Tables tb, int descramble, ListQueue *ql, ListSlot *slots_l, float *llr_l, int *slot_of, int chunk_seq = 0);
void launch_sc_adapt(hipStream_t s, ListQueue *qs);
size_t sc_store_bytes(int lb);  // level store per resident decoder
int sc_codewords_per_wave(int lb);
// D9 / D10 for the run `par` of the queue; grid = resident decoders, max_entries = an upper bound of the run's length
void launch_polar(hipStream_t s, int list, int grid, ListQueue *q, int par, const ListSlot *slots, const float *llr_q, float *soft, uint8_t *hard_q,
	Tables tb, float *metric_q);
void launch_finish(hipStream_t s, int list, int max_entries, const ListQueue *q, int par, const ListSlot *slots, const float *llr_q,
	const uint8_t *hard_q, Tables tb, int descramble, uint8_t *lane_mesg_q, int lane_mesg_stride);   // (stride: bytes per lane of the debug copy)
void launch_fft_debug(hipStream_t s, int rate, int n, int len, int sign, const cf *in, cf *out, Tables tb);
void launch_awgn_tile(hipStream_t s, const int16_t *base, size_t n_base, int16_t *out, size_t n_out,
	size_t spf, float sigma, uint64_t seed, uint64_t first_frame);
void launch_channel(hipStream_t s, int rate, const int16_t *in, int16_t *out, size_t n, size_t spf, const void *params);
size_t fading_tile_samples();   // samples per workgroup of k_fading: the launch holds 65535 of them per frame
void launch_fading(hipStream_t s, int rate, const int16_t *in, size_t n_in, int16_t *out, size_t n_out, size_t spf, const void *params,
	uint64_t seed, uint64_t first_frame);
size_t tx_big_scratch_bytes(int rate, int n, int nsym);
void launch_tx(hipStream_t s, int rate, int n, const uint8_t *payload, Tables tb, const void *tp, const cf *tw_sym4,
	uint32_t *code, cf *rowsym, cf *tdom, cf *big_scratch, void *pcm);
// chunk_flags (nullable): per-chunk device flags cleared here ([0]: the largest row count k_theil_sen met, when above 50)
void launch_init_sync(hipStream_t s, int n, SyncState *st, const int32_t *skip_counts, int *chunk_flags = nullptr, int32_t *attempt_counts = nullptr);

// ---- stream decode (k_stream.hip, api_streams.cpp): every preamble of every recording of a call - one
// recording is a batch of one.  The timing metric is formed tile by tile (STREAM_TILE sample times per workgroup), the trigger
// (decode.cc:93-116) resolved by a scan over the tiles: each tile publishes what it does to an incoming (Schmitt state, running
// maximum since the last falling edge, edge count) for either incoming state, one workgroup per recording scans those functions,
// and the tiles then emit their falling edges in stream order.
constexpr int STREAM_TILE = 4096;
struct StreamFn {                  // a tile (or a run of tiles) as a function of the incoming Schmitt state s = 0 / 1
	int s_out[2];                  // the state after it
	int has[2];                    // it holds a falling edge
	long long n[2];                // falling edges in it
	float m[2];                    // maximum of the timing metric since its last falling edge (all of it if none), first index of it
	long long i[2];
};
struct StreamCarry { int s; float m; long long i; long long count; };   // what enters a tile
struct StreamEdge {                // one falling edge, in stream order
	long long g, t_max;            // the edge sample, the first index of the maximum of its run
	int index_max;                 // decode.cc:99-105
	int accept;                    // decode.cc:110-151 (k_stream_accept)
	int symbol_pos;                // window coordinate after pos_err, when accepted
	float cfo_rad;
};
// The recording is the second grid dimension.  Every recording is scanned from its own position 0 with its own tile count, and
// nothing crosses from one to the next: what enters tile 0 of each is the initial state.  fb.tile0 places a recording's tiles in
// tile_end / tile_in / fn / carry; ck is [n_src][ck_per_src], z [n_src][fb.samples_per_frame], edges [n_src][cap], counts
// [n_src][2] (falling edges, accepted preambles).  max_len: the longest recording (the grids' first dimension).  The caller clears
// counts before launch_streams_scan: a recording without tiles writes none
// _dc: mono input: the DC blocker's kept states of every recording (the layout of k_mono_carries, a recording as a frame) by a scan
// over tiles of 4096 samples; tile_end / tile_in: one double per tile
// _scan: the trigger scan over the 2-channel recordings fb (given != nullptr: over those timing sequences instead, packed from
// fb.given0); counts[q][0]: falling edges; edges: the first `cap` of them
// _accept: decode.cc:110-151 for every edge (of the min(counts[q][0], cap) written)
void launch_streams_dc(hipStream_t s, int n_src, long max_len, SourceBatch fb, FrontCoef co, double *tile_end, double *tile_in, double *ck, int ck_per_src);
void launch_streams_front(hipStream_t s, int rate, int n_src, long max_len, SourceBatch fb, MonoArgs ma, cf *z);
void launch_streams_scan(hipStream_t s, int rate, int n_src, long max_len, SourceBatch fb, const float *given, StreamFn *fn, StreamCarry *carry,
	StreamEdge *edges, long cap, long long *counts);
void launch_streams_accept(hipStream_t s, int rate, int n_src, SourceBatch fb, Tables tb, StreamEdge *edges, long cap, long long *counts);
// the records: counts[q][1] = accepted edges; first[q] (n_src + 1): where recording q's records begin in the packed order, a running
// sum of min(accepted, max_per_src); rec / rec_src: for every packed record below max_rec, the SyncState that k_header finds for
// that accepted edge after a round with skip_left = 0, and the recording it reads
void launch_streams_records(hipStream_t s, int rate, int n_src, const StreamEdge *edges, long cap, long long *counts, long long *first,
	SyncState *rec, int *rec_src, long long max_per_src, long long max_rec);


// ---- live channels (api_bank.cpp; a feed is a bank of one channel): the same kernels over a WINDOW of every
// channel's stream, with the channel as the second grid dimension.  A channel's samples (and ck, z) are addressed from where its
// position 0 would lie - its place in the slab minus its window's base - with the samples fed so far as its length; the host checks
// before every launch that the window holds every position the launch reads below that.
// Every array is per channel: edges [n_ch][cap], counts [n_ch][2], c_in / c_out [n_ch] (a channel without tiles in this push keeps
// its carry).  max_tiles: the most tiles any channel brings (the grids' first dimension).  The caller clears counts and fb.below.
// The scan of channel q takes its tiles fb.tile0[q] .. from the carry c_in[q] (count taken as 0) and leaves c_out[q] behind them;
// counts[q][0]: their edges.  fb.below[q] is set when an edge would read below fb.lo[q] (it is then left rejected: an internal error)
void launch_bank_scan(hipStream_t s, int rate, int n_ch, long max_tiles, WindowBatch fb, StreamFn *fn, StreamCarry *carry, const StreamCarry *c_in,
	StreamCarry *c_out, StreamEdge *edges, long cap, long long *counts);
void launch_bank_accept(hipStream_t s, int rate, int n_ch, WindowBatch fb, Tables tb, StreamEdge *edges, long cap, long long *counts);
// the packed records of the push in channel order: first [n_ch + 1] as launch_streams_records; record indices count from rec_base[q],
// rejects from rej_base[q]; only the first max_rec are written
void launch_bank_records(hipStream_t s, int rate, int n_ch, const StreamEdge *edges, long cap, long long *counts, long long *first, SyncState *rec,
	int *rec_src, const long long *rec_base, const long long *rej_base, long long max_rec);
// planes x n_ch byte ranges copied in one launch: range (p, q), at index p * plane_stride + q of the three arrays, is bytes[] bytes
// from the address src[] to the address dst[], which are the same modulo 16 (the window move: both multiples of 16; the new
// samples: packed that way by the host).  max_bytes: the longest range
void launch_bank_copy(hipStream_t s, int n_ch, int planes, size_t plane_stride, long long max_bytes, const long long *src, const long long *dst,
	const long long *bytes);
// mono input: the DC blocker and the front end over the windows.  Channel q's DC blocker resumes at fb.dc_from[q] (a multiple of 64,
// from the state kept before it) with fb.dc_at[q + 1] - fb.dc_at[q] tiles (tile_end / tile_in: at fb.dc_at[q]) and keeps the states
// of the complete blocks; its front end forms the stretches fb.fe0[q] .. (k_sync.hip: front_end_stretch() samples each, from position
// 0), fb.fe_at[q + 1] - fb.fe_at[q] of them.  ck, z (ma.ck likewise): the slabs fb.ck_org / fb.z_org count from
long front_end_stretch();
void launch_bank_dc(hipStream_t s, int n_ch, long max_tiles, WindowBatch fb, FrontCoef co, double *tile_end, double *tile_in, double *ck);
void launch_bank_front_end(hipStream_t s, int rate, int n_ch, long max_stretch, WindowBatch fb, MonoArgs ma, cf *z);

// ---- the wideband front end (k_channelize.hip): mix-down, FIR and decimation by p / q
// (in lowest terms, 1 <= q <= 16, 2 <= p / q <= 32; q = 1: the integer decimation D = p) of one wideband capture into n_channels
// channel rows.  in: wideband positions in_first .. in_first + n_in - 1 (interleaved I/Q of fmt); every position outside reads as
// zero and is never loaded.  Output n of channel c (n = out_first .. out_first + n_out - 1) reads the wideband positions
// n p div q - (T - 1) .. n p div q, T = 24 p div q + 1, and goes to out + 2 (c out_stride + n - out_first) floats, or
// - dst != nullptr - to the address dst[c] + 8 (n - out_first) (the bank: every channel's place in its window).  taps: device,
// [T][q] - tap j of phase r at j q + r, the transpose of what rechannelize_taps writes (q = 1: the T taps of channelize_taps as
// they are); inc: the channels' phase increments.
struct ChannelizeArgs {
	const void *in;
	int fmt;                       // OFDMRX_FMT_*
	int p, q;
	long long in_first, n_in;
	const float *taps;             // device, [T][q]
	const unsigned *inc;           // device, [n_channels]
	int n_channels;
	long long out_first, n_out;    // n_out <= channelize_max_outputs(q)
	float *out;
	long long out_stride;          // I/Q pairs per channel row
	const long long *dst;          // device, [n_channels] addresses, nullable
	// the grid front end (k_channelize_grid.hip): grid != 0, q = 1, p = D a power of two 2 .. 512, M = 2 D; channel c is
	// slot k_c = inc[c] >> (32 - log2 M) (inc[c] = k_c 2^32 / M mod 2^32: the increment of its centre k_c rate / 2, exactly);
	// tw: device, the M / 2 roots e^{+2 pi i j / M}, rounded once from double
	int grid;
	const float2 *tw;
	// a REAL capture: real != 0, grid == 0; in holds ONE value of fmt per wideband position
	int real;
};
// a.grid == 0: k_channelize where a.q == 1, k_rechannelize otherwise - each keeps its own summation order (see the file) - for an
// analytic capture or, a.real != 0, a real one: the same sums on the capture (x, +0), doubled, byte for byte.  A real capture's
// tiles are no shorter than an analytic one's, so channelize_max_outputs bounds n_out for both
void launch_channelize(hipStream_t s, const ChannelizeArgs &a);
long long channelize_max_outputs(int q);
void launch_channelize_grid(hipStream_t s, const ChannelizeArgs &a);    // k_channelize_grid.hip: a.grid != 0 (the callers choose)
// log2 M of the grid's D = 2, 4 .. 512 (M = 2 D), for the front end, the synthesizer and the survey; D must be one of those powers of
// two (channelize_grid_decim): any other D is rounded up to the next, which is not its transform
constexpr int grid_logm(int D)
{
	int logm = 1;
	while ((1 << logm) < 2 * D)
		++logm;
	return logm;
}
long long channelize_grid_max_outputs();
// the grid front end at a ratio (k_channelize_grid_ratio.hip): a.grid == 2, p / q in lowest terms with p = 2^a 3^b 5^c
// (not q = 1 with p a power of two: that is 4.19's kernel), M = 2 p; taps as k_rechannelize reads them; tw: device, the M
// roots e^{-2 pi i j / M}, rounded once from double; channel c is slot k_c with
// inc[c] = channelize_grid_ratio_row(plan, (-k_c q) mod M) | (k_c q mod M) << 16
struct GridRatioPlan {
	int m, n_taps;                 // M = 2 p, T = 24 p div q + 1
	int nt;                        // output times per tile
	int ch, groups;                // times per run of the branch sums (1, 2, 4, 8 or 16), runs per residue of 2 q
	unsigned radices;              // the transform's stages, four bits each, the first lowest: every 5, every 3, every 4, a last 2
	size_t lds;                    // dynamic LDS in bytes
};
GridRatioPlan channelize_grid_ratio_plan(int p, int q);
void channelize_grid_ratio_runs(GridRatioPlan &pl, int q);   // ch and groups for pl.nt, pl.m and pl.n_taps (the survey's tile differs)
int channelize_grid_ratio_row(const GridRatioPlan &pl, int bin);   // where a bin stands behind the transform
void launch_channelize_grid_ratio(hipStream_t s, const ChannelizeArgs &a);
long long channelize_grid_ratio_max_outputs();
// host: the taps of decimation D (T = 24 D + 1 of them; returns T) and the phase increment of a centre frequency at wideband rate rw
int channelize_taps(int decim, float *taps);
unsigned channelize_inc(double centre_hz, double rw);
// host: the taps of the reduced ratio p / q as [q][T] (returns T); q = 1: channelize_taps(p, .)
int rechannelize_taps(int p, int q, float *taps);

// ---- the wideband synthesizer (k_synthesize.hip, k_resynthesize.hip): n_channels narrowband rows -> one
// wideband capture at p / q times their rate (lowest terms, 1 <= q <= 16, 2 <= p / q <= 32; q = 1: the integer interpolation p).
// in: sample frame j (0 .. n_in - 1) of channel c at c in_stride + j sample frames (interleaved I/Q of in_fmt: S16 or F32); every
// index outside reads as zero and is never loaded.  Output m (out_first .. out_first + n_out - 1) goes m - out_first sample frames
// into out, as out_fmt (S16 or F32).  taps: device; q = 1: the 24 p + 1 fp32 taps of channelize_taps; q > 1: 16-byte aligned,
// [p][RSY_ROW] - row b holds G[b + a p], a = 0 .. 24, of the sequence G[tn] = H[tn mod q][tn div q], tn = 0 .. 24 p, that
// rechannelize_taps' table [q][T] spells, zeros behind it (resynthesize_taps writes it).
constexpr int RSY_ROW = 28;
struct SynthChannel {
	long long start;               // wideband index of the channel's first input sample, >= 0
	unsigned inc;                  // channelize_inc of its centre
	float gain;                    // p / q x the caller's gain, rounded once
};
struct SynthesizeArgs {
	const void *in;
	int in_fmt, out_fmt;           // OFDMRX_FMT_S16 or OFDMRX_FMT_F32
	int p, q;
	long long in_stride, n_in;     // sample frames
	const SynthChannel *ch;        // device, [n_channels]
	const float *taps;             // device
	int n_channels;
	long long out_first, n_out;    // n_out <= synthesize_max_outputs(q)
	void *out;
};
// k_synthesize where a.q == 1, k_resynthesize (launch_synthesize_ratio) otherwise: they tile differently (profiles/resynthesize.txt)
void launch_synthesize(hipStream_t s, const SynthesizeArgs &a);
void launch_synthesize_ratio(hipStream_t s, const SynthesizeArgs &a);   // k_resynthesize.hip: launch_synthesize's q > 1
long long synthesize_max_outputs(int q);

// ---- the wideband synthesizer on a channel grid (k_synthesize_grid.hip): n_channels rows, row c in slot
// k_c = ch[c].inc >> (32 - log2 M) (inc = k_c 2^32 / M mod 2^32, as in 4.19), ch[c].start a multiple of D = p, the slots pairwise
// distinct -> one wideband capture at D times their rate.  One launch makes a chunk of output times q = q_first .. q_first + nq - 1
// (output m belongs to time m div D) and writes the outputs of those times that lie in out_first .. out_first + n_out - 1.
// scratch: device, n_times M float2 - V of the absolute input times j_first = q_first - 24 .. j_first + n_times - 1 as [time][r];
// n_times is a multiple of synthesize_grid_tile_times(D) and at least nq rounded up to 8, plus 24.
struct SynthesizeGridArgs {
	const void *in;
	int in_fmt, out_fmt;           // OFDMRX_FMT_S16 or OFDMRX_FMT_F32
	int p;                         // D, a power of two 2 .. 512
	long long in_stride, n_in;     // sample frames
	const SynthChannel *ch;        // device, [n_channels]
	const float *taps;             // device, the 24 D + 1 taps of channelize_taps
	const float2 *tw;              // device, the M / 2 roots e^{+2 pi i j / M}, rounded once from double
	int n_channels;
	long long out_first, n_out;
	void *out;
	float2 *scratch;
	long long j_first, q_first;
	int n_times, nq;
};
// the transform kernel over the scratch's n_times, then the filter kernel over the chunk's nq
void launch_synthesize_grid(hipStream_t s, const SynthesizeGridArgs &a);
int synthesize_grid_tile_times(int interp);     // input times per workgroup of the transform kernel
int synthesize_grid_filter_times(int interp);   // output times per workgroup of the filter kernel

// ---- the grid synthesizer at a ratio (k_synthesize_grid_ratio.hip): p / q in lowest terms with p = 2^a 3^b 5^c (not
// q = 1 with p a power of two: that is 4.20's kernels), M = 2 p.  Row c is slot k_c with
//   ch[c].start = sigma_c q, the absolute input time of its first sample (the caller's start is sigma_c p)
//   ch[c].inc   = channelize_grid_ratio_row(plan, (-k_c) mod M) | (k_c mod 2) << 16
//   ch[c].gain  = p / q x the caller's gain, rounded once
// taps: 16-byte aligned, [p][RSY_ROW] as launch_synthesize_ratio reads them; tw: the M roots e^{-2 pi i j / M}, rounded once from
// double.  One launch makes the chunk's outputs m_first .. m_first + n_m - 1, which lie inside out_first .. out_first + n_out - 1.
// scratch: device, n_times M float2 - V of the absolute input times j_first .. j_first + n_times - 1 as [time][r]; j_first =
// (m_first q) div p - 24, n_times a multiple of synthesize_grid_ratio_tile_times(p, q) that holds ((m_first + n_m - 1) q) div p - at
// q = 1, where the filter's work items take synthesize_grid_ratio_filter_round(1) = 8 output times each, the chunk's number of output
// times rounded up to 8, plus 24.
struct SynthesizeGridRatioArgs {
	const void *in;
	int in_fmt, out_fmt;           // OFDMRX_FMT_S16 or OFDMRX_FMT_F32
	int p, q;
	long long in_stride, n_in;     // sample frames
	const SynthChannel *ch;        // device, [n_channels]
	const float *taps;
	const float2 *tw;
	int n_channels;
	long long out_first, n_out;
	void *out;
	float2 *scratch;
	long long j_first, m_first, n_m;
	int n_times;
	int m, nt;                     // the launcher fills these three in from channelize_grid_ratio_plan(p, q)
	unsigned radices;
};
void launch_synthesize_grid_ratio(hipStream_t s, const SynthesizeGridRatioArgs &a);
int synthesize_grid_ratio_tile_times(int p, int q);   // input times per workgroup of the transform kernel
int synthesize_grid_ratio_filter_outputs(int p, int q);   // outputs per workgroup of the filter kernel
int synthesize_grid_ratio_filter_round(int q);        // output times per work item of the filter kernel (q > 1: 1)

// ---- the wideband survey (k_survey.hip): a Welch power spectrum of one wideband capture, n_rows rows of nfft bins.
// in: wideband positions in_first .. in_first + n_in - 1 (interleaved I/Q of fmt); the caller has checked that every position the
// rows need is there.  Row r (row_first .. row_first + n_rows - 1) averages the segs_per_row segments from r segs_per_row on, in
// groups of SURVEY_G: k_survey leaves the partial of (row, group) at part + ((r - row_first) n_groups + group) nfft floats in
// natural bin order, k_survey_rows sums the groups in ascending order, multiplies by scale and writes row r in ascending frequency
// at out + (r - row_first) nfft.  win: the nfft fp32 window values; tw: the nfft roots e^{-2 pi i m / nfft}.
constexpr int SURVEY_G = 8;            // segments per group: part of the definition's summation order
struct SurveyArgs {
	const void *in;
	int fmt;                       // OFDMRX_FMT_*
	int nfft;                      // 1280, 2560 or 5120
	long long in_first, n_in;
	int segs_per_row;              // 1 .. 65536
	int n_groups;                  // ceil(segs_per_row / SURVEY_G)
	long long row_first, n_rows;   // n_rows n_groups nfft <= survey_max_partial_floats()
	const float *win;              // device
	const cf *tw;                  // device
	float *part;                   // device, n_rows n_groups nfft floats
	float *out;
};
void launch_survey(hipStream_t s, const SurveyArgs &a, float scale);
inline long long survey_max_partial_floats() { return 1LL << 28; }   // the partials of one call: 1 GiB at most
// host: the periodic Hann window of nfft points, rounded once to fp32 (returns nfft)
int survey_window(int nfft, float *w);

// ---- the grid survey (k_survey_grid.hip): the mean power of every slot of the grid front end's bank (4.19), n_rows
// rows of M = 2^logm = 2 D slots.  in: wideband positions in_first .. in_first + n_in - 1 (interleaved I/Q of fmt); a position below
// 0 reads as zero, and the caller has checked that every other position the rows need is there.  The call covers the absolute output
// times t_first = row_first S .. t_first + n_times - 1, n_times = n_rows S, S a multiple of SURVEY_GRID_G: k_survey_grid leaves the
// power of group j (the times t_first + 8 j ..) at part + j M floats in the order of the transform's output (slot k mod M at
// brev(k mod M)); k_survey_grid_rows sums a row's n_groups = S / 8 groups in ascending order, multiplies by scale and writes row r
// in ascending slot order at out + (r - row_first) M.  taps, tw: the grid table of 4.19 (ChannelizeArgs).
constexpr int SURVEY_GRID_G = 8;       // output times per group: part of the definition's summation order
struct SurveyGridArgs {
	const void *in;
	int fmt;                       // OFDMRX_FMT_*
	int logm;                      // 2 .. 10
	long long in_first, n_in;
	const float *taps;             // device, the 24 D + 1 taps
	const float2 *tw;              // device, the M / 2 roots e^{+2 pi i j / M}
	long long t_first, n_times;
	int n_groups;                  // S / 8
	long long n_rows;              // n_rows n_groups M <= survey_max_partial_floats()
	float *part;                   // device, n_rows n_groups M floats
	float *out;
};
void launch_survey_grid(hipStream_t s, const SurveyGridArgs &a, float scale);

// ---- the grid survey at a ratio (k_survey_grid_ratio.hip): the mean power of every slot of the ratio grid front
// end's bank (4.22), n_rows rows of n_all slots, p / q in lowest terms with p = 2^a 3^b 5^c (not q = 1 with p a power of two: that is
// 4.21's kernel).  in, in_first, n_in, t_first, n_times, n_groups, n_rows: as SurveyGridArgs.  taps, tw, inc: the ratio-grid table
// of 4.22 with every slot in ascending order, inc[c] & 0xffff the LDS row of slot k_first + c.  k_survey_grid_ratio leaves the power
// of group j at part + j n_all floats in slot order; k_survey_grid_ratio_rows sums a row's groups in ascending order, multiplies by
// scale and writes row r at out + (r - row_first) n_all.
struct SurveyGridRatioArgs {
	const void *in;
	int fmt;                       // OFDMRX_FMT_*
	int p, q;
	long long in_first, n_in;
	const float *taps;             // device, [T][q]
	const float2 *tw;              // device, the M roots e^{-2 pi i j / M}
	const unsigned *inc;           // device, [n_all]
	int n_all;
	long long t_first, n_times;
	int n_groups;                  // S / 8
	long long n_rows;              // n_rows n_groups n_all <= survey_max_partial_floats()
	float *part;                   // device, n_rows n_groups n_all floats
	float *out;
};
// the front end's plan with the survey's own tile, a multiple of 8 (the tile enters no output)
GridRatioPlan survey_grid_ratio_plan(int p, int q);
// (an error only where the runtime refuses more than 64 KiB of dynamic LDS: the 8-time tile at M >= 960)
hipError_t launch_survey_grid_ratio(hipStream_t s, const SurveyGridRatioArgs &a, float scale);

}  // namespace rx
