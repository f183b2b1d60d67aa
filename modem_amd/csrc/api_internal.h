// api_internal.h -- what the files of the C ABI share: the handle, its buffers, the helpers that cross files.
// (round 6: ofdmrx_api.cpp was one file of 1700 lines - api_create.cpp / api_pipeline.cpp / api_debug.cpp / api_tx.cpp now)
#pragma once
#include "../../include/ofdmrx.h"
#include "kernels.h"
#include "tables.h"
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace rx;


static_assert(sizeof(Result) == sizeof(ofdmrx_frame_result), "Result must mirror ofdmrx_frame_result");
static_assert(sizeof(Attempt) == sizeof(ofdmrx_attempt) && ATTEMPTS_MAX == OFDMRX_MAX_SKIP + 1, "Attempt must mirror ofdmrx_attempt");


extern thread_local std::string g_last_error;   // (api_create.cpp)

struct DevBuf {                    // owns its device memory: a buffer of the handle goes with the handle, a local one with its scope
	void *p = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { release(); }
	int ensure(size_t need)
	{
		if (need <= bytes)
			return 0;
		release();
		hipError_t e = hipMalloc(&p, need);
		if (e != hipSuccess) {
			g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
			return OFDMRX_E_NOMEM;
		}
		bytes = need;
		return 0;
	}
	void release()
	{
		if (p)
			(void)hipFree(p);
		p = nullptr;
		bytes = 0;
	}
	template <typename T> T *as() const { return (T *)p; }
};

// Where a decode call's outputs go: the arrays of include/ofdmrx.h for its frames, all in ONE memory space (HBM, or pinned host
// memory).  The public entries build it once, from their arguments and what ofdmrx_set_esn0_rows / ofdmrx_set_attempt_log left in
// the handle; everything below takes it by value.
struct Outputs {
	uint8_t *payload = nullptr;    // n x PAYLOAD_BYTES
	Result *res = nullptr;
	float *esn0 = nullptr;         // n x ROWS_MAX, or null: off
	Attempt *att = nullptr;        // n x ATTEMPTS_MAX and n counts, or both null: off
	int32_t *att_counts = nullptr;
	Outputs from(size_t first) const   // the same arrays, starting at frame `first`
	{
		return { payload + first * PAYLOAD_BYTES, res + first, esn0 ? esn0 + first * ROWS_MAX : nullptr,
			att ? att + first * ATTEMPTS_MAX : nullptr, att ? att_counts + first : nullptr };
	}
};

inline size_t sample_bytes(int fmt) { return fmt == OFDMRX_FMT_S16 ? 2 : fmt == OFDMRX_FMT_U8 ? 1 : 4; }
// what every decode entry asks of its samples: a known format, one or two channels (decode.cc:578), and a start on a sample-frame
// boundary - the kernels load I/Q pairs with one access
inline int check_samples(const void *samples, int fmt, int channels)
{
	if (!samples || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || channels < 1 || channels > 2)
		return OFDMRX_E_ARG;
	return (size_t)samples % (sample_bytes(fmt) * (size_t)channels) ? OFDMRX_E_ARG : 0;
}

// ---- optional roctx ranges around the stage launches (OFDMRX_ROCTX=1): markers for rocprofv3 --marker-trace.
// The library is looked up at run time, so libofdmrx.so keeps its single dependency (libamdhip64).
struct Roctx {
	int (*push)(const char *) = nullptr;
	int (*pop)() = nullptr;
	Roctx()
	{
		if (!std::getenv("OFDMRX_ROCTX"))
			return;
		for (const char *name : { "librocprofiler-sdk-roctx.so", "libroctx64.so" }) {
			if (void *lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
				push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
				pop = (int (*)())dlsym(lib, "roctxRangePop");
				if (push && pop)
					return;
			}
		}
		push = nullptr;
		pop = nullptr;
	}
};
struct Range {                     // RAII: one named range per stage of a chunk
	static Roctx &api() { static Roctx r; return r; }
	explicit Range(const char *name) { if (api().push) api().push(name); }
	~Range() { if (api().pop) api().pop(); }
};

// call sign -> base-37 integer (the encoding of encode.cc:320-335: ' ' = 0, '0'..'9' = 1..10, letters of either case
// = 11..36); -1 for any other character
inline long long callsign_value(const char *str)
{
	static const std::array<int8_t, 256> digit = [] {
		std::array<int8_t, 256> t{};
		t.fill(-1);
		t[(unsigned char)' '] = 0;
		for (int i = 0; i < 10; ++i)
			t[(unsigned char)('0' + i)] = (int8_t)(1 + i);
		for (int i = 0; i < 26; ++i)
			t[(unsigned char)('A' + i)] = t[(unsigned char)('a' + i)] = (int8_t)(11 + i);
		return t;
	}();
	long long acc = 0;
	for (; *str; ++str) {
		const int d = digit[(unsigned char)*str];
		if (d < 0)
			return -1;
		acc = acc * 37 + d;
	}
	return acc;
}



static constexpr int T_SC = OFDMRX_T_COUNT;   // internal stage index of the list-1 pass

struct ofdmrx_handle {
	ofdmrx_config cfg;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	int chunk = 0;
	long max_samples = 0;
	int rate = 8000;
	int list = 8;             // SCL list size: 8 (AVX2 build of the reference) or 4 (decode.cc:164-169)
	HostTables host;
	Tables dev{};
	std::vector<void *> table_allocs;
	// per-chunk device state: one buffer each - every stage from the scan to k_back runs on the handle's stream, chunk after
	// chunk; what crosses to the list decoder's streams goes through the queue below
	int cap = 0;              // frames the buffers below are sized for
	long cap_samples = 0;     // samples per frame the mono buffers are sized for
	DevBuf st, hdr_soft, cons, slope, yint, precision, slot_of;
	DevBuf payload[2], res[2];   // device-side output staging by chunk parity (host-pointer entry, pinned outputs); [0]: the debug entries' outputs
	DevBuf chunk_flags;       // per-chunk device flags (k_theil_sen: the largest row count met)
	DevBuf soft;              // the level stores of the resident list decoders (2 MiB each)
	// the list decoder's work queue (kernels.h: ListQueue): control block + one slot per entry
	DevBuf q_ctl, q_slots, q_llr, q_hard, q_metric, q_lane_mesg;
	unsigned q_cap = 0;       // slots
	// the SC ring in front of it (k_sc.hip): control block, one slot per frame of a chunk (LLRs, P*'s codeword, the channel's hard
	// decisions, ScStat), one level store per resident decoder
	DevBuf s_ctl, s_slots, s_llr, s_cw, s_xw, s_stat, sc_soft;
	unsigned s_cap = 0;
	unsigned sc_unit = 1;     // entries a run of the list-1 pass takes at a time: one residency of its decoders (the last run of a call: everything)
	int sc_mode = 1;          // 1: the list-1 pass (adaptive) in front of the list decoder, 0: off
	int sc_grid = 0, sc_grid6 = 0;   // resident SC decoders (waves): two codewords per wave / one (k_sc.hip)
	int sc_top = 1;           // k_sc skips clean nodes of 16384 / 32768 leaves on a lower bound of their share of min_fork (OFDMRX_SC_TOP=0: every figure exact)
	int sc_lb = 6;            // one codeword per wave (6, the default: with 64 loads in flight it is the faster layout at every run length, and
	                          // it moves 2.1 MB per codeword against 2.7), two (5), or 0: the run's length picks on the device (OFDMRX_SC_LB)
	ListQueue *sc_queue() const { return s_ctl.as<ListQueue>(); }
	ScRing sc_ring() const { return sc_mode ? ScRing{ s_ctl.as<ListQueue>(), s_slots.as<ListSlot>(), s_llr.as<float>() } : ScRing{ nullptr, nullptr, nullptr }; }
	unsigned flush_unit = 1;  // entries a flush takes at a time (one residency of the list decoder) unless it is forced
	DevBuf rot_tap;           // OFDMRX_TAP_CONS_ROT: the rotated rows of one frame, made on demand
	DevBuf tx_code, tx_rowsym, tx_tdom, tx_big;   // transmitter scratch, kept between calls (no allocation, no synchronisation per call)
	hipStream_t stream_b = nullptr;     // the list decoder (k_polar) of chunk c - 1 runs here beside the front stages of chunk c
	hipStream_t stream_fin = nullptr;   // k_finish (+ the host entry's output copies) of chunk c - 2
	hipStream_t stream_c = nullptr;     // host-pointer entry: host-to-device copies of the next chunk
	hipError_t sticky = hipSuccess;   // first failed hipEventRecord of the running call
	int polar_grid = 0;       // resident list decoders
	int cert_mode = 1;        // 1: syndrome certificate (adaptive), 0: every frame with a header is list-decoded
	float *esn0_user = nullptr;   // ofdmrx_set_esn0_rows: n x OFDMRX_ROWS_MAX floats in the memory space of the results (NULL = off)
	DevBuf esn0_dev[2];           // host-pointer entry: per-chunk device staging of the row values, by parity
	ofdmrx_attempt *att_user = nullptr;   // ofdmrx_set_attempt_log: n x (OFDMRX_MAX_SKIP + 1) records and n counts, same memory space (NULL = off)
	int32_t *att_counts_user = nullptr;
	DevBuf att_dev[2], attc_dev[2];   // host-pointer entry: their device staging, by parity
	ListQueue *queue() const { return q_ctl.as<ListQueue>(); }
	DevBuf dc, z;             // mono front end only
	long last_spf = 0;
	DevBuf in_stage[2], skip_stage;   // host-pointer entry: the samples of a chunk, by parity; the call's SKIP counts
	void *out_stage[2] = { nullptr, nullptr };   // pinned host staging of payloads + results (host-pointer entry)
	size_t out_stage_cap[2] = { 0, 0 };
	DevBuf carr;                   // payload carriers of every symbol (demod -> Theil-Sen) at the rates whose demodulator does not form the rows
	DevBuf sc_scratch;             // rates above 8 kHz: 2 x symbol_len/2 cf per frame for the S&C trigger part
	int last_n = 0;           // frames in the last chunk (for taps)
	size_t last_first = 0;    // index of that chunk's first frame in its call (ofdmrx_last_chunk_first_frame)
	bool last_mono = false;
	FrameBatch last_fb{};     // the last chunk's samples (the ANALYTIC tap forms its frame's analytic signal from them)
	// timing
	std::vector<hipEvent_t> ev_pool;
	size_t ev_used = 0;
	struct Span { int stage; size_t a, b; };
	std::vector<Span> spans;
	ofdmrx_timing timing{};
	float sc_ms = 0.f;        // the list-1 pass (stage T_SC: ofdmrx_timing keeps its layout, ofdmrx_get_sc_timing reports it)
	int sc_launches = 0;
	// Two lanes (round 6, opt-in: OFDMRX_FLAG_TWO_LANES / OFDMRX_LANES=2): a device-entry call of four chunks or more is cut in two,
	// the second half runs through a second pipeline of the same configuration - `lane2`, a handle of its own with its own streams
	// and state - beside the first.  Kernels of the two lanes fill each other's gaps - the tail of a k_sc run in which most
	// persistent decoders have run out of codewords, the dispatch ramp of every launch: -20 dB 816 -> 850 - 865 k frames/s,
	// configs[3] 892 -> 950 - 990 k, -26 dB 1.42 -> 1.56 M.  Where the syndrome certificate finishes every frame there is nothing
	// to share (the front kernels are bound by vector issue): 1.82 M with one lane, 1.79 - 1.80 M with two - hence opt-in.  It needs
	// hardware queues of its own: HIP maps streams onto GPU_MAX_HW_QUEUES of them (default 4) and kernels of streams that share
	// one run in order (with 4 the lanes mostly alternate: 794 k at -20 dB).  profiles/r06_hw_queues_and_two_lanes.txt
	ofdmrx_handle *lane2 = nullptr;
	int lanes = 1;
	size_t split_at = 0;      // frames of the last call that went through this handle's own pipeline (0: all of them)
	hipEvent_t ev_lane_in = nullptr, ev_lane_done = nullptr;
	// stream decode (api_streams.cpp; the live entries of api_bank.cpp share the output staging): scratch kept between calls, grown on demand
	DevBuf sx_in, sx_z, sx_ck, sx_dc_end, sx_dc_in, sx_fn, sx_carry, sx_edges, sx_counts, sx_rec, sx_pay, sx_res, sx_esn0, sx_timing;
	// ... the per-recording lengths and tile places, the packed order, the record -> recording map
	DevBuf sxs_len, sxs_tile0, sxs_given0, sxs_first, sxs_rec_src;
	std::vector<int> sxs_len_h;           // (host copies the uploads read: they live as long as the handle)
	std::vector<long long> sxs_tile0_h, sxs_given0_h, sxs_counts_h;
	long sxs_edge_cap = 0;    // every recording's share of the edge buffer (one recording: all of it)
	struct ofdmrx_bank *bank = nullptr;   // the open bank of live channels or - a bank of one - the open feed (api_bank.cpp): one per handle
	bool busy_live() const { return bank != nullptr; }   // a handle with an open feed or bank decodes nothing else
	// the wideband front end (api_channelize.cpp): the taps [T][q] and the phase increments on the device, and what they were made
	// from - the reduced ratio chz_p / chz_q (an integer decimation D is D / 1; 0 / 0: none) and the host copies the uploads read
	DevBuf chz_taps, chz_inc;
	int chz_p = 0, chz_q = 0;
	int chz_grid = 0;                    // the table is a grid table: the roots of the transform stand behind the taps (at chz_tw_at floats); 2: a ratio-grid table (4.22)
	size_t chz_tw_at = 0;
	std::vector<float> chz_taps_h;
	std::vector<unsigned> chz_inc_h;
	// the wideband synthesizer (api_synthesize.cpp): a small ring of parameter sets - the channels' (start, inc, gain) and the taps
	// behind them - so that a call with other parameters never writes what a launch still in flight reads: a slot is written again
	// only after the event of its last launch
	struct SynSlot {
		DevBuf dev;
		std::vector<SynthChannel> ch;   // (the host copy the upload reads: it lives as long as the slot)
		std::vector<float> taps;
		int p = 0, q = 0;               // the reduced ratio the set was made for (q = 1: the integer synthesizer's interp); 0: none
		int grid = 0;                   // 1: a grid set: inc spells the slot, the M / 2 roots stand behind the taps (at tw_at floats); 2: a ratio-grid set (4.23)
		size_t tw_at = 0;
		hipEvent_t done = nullptr;
		~SynSlot() { if (done) (void)hipEventDestroy(done); }
	};
	SynSlot syn[4];
	int syn_cur = 0;
	DevBuf syn_scratch;                  // the grid synthesizer's V of one chunk (api_synthesize.cpp: SYG_SCRATCH_BYTES at most)
	// the wideband survey (api_survey.cpp): per transform length (1280, 2560, 5120) the window and the roots on the device, uploaded
	// on the first call with that length and never written again; the partials of the last call (grown on demand)
	struct SurveyPlan {
		DevBuf win, tw;
		std::vector<float> win_h;   // (the host copies the uploads read: they live as long as the handle)
		std::vector<cf> tw_h;
		double u = 0.0;             // sum of the squared fp32 window values
	};
	SurveyPlan survey[3];
	DevBuf survey_part;
};

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
	g_last_error = std::string(#call) + ": " + hipGetErrorString(e_); return OFDMRX_E_HIP; } } while (0)

template <typename T>
static int upload(ofdmrx_handle *h, const std::vector<T> &v, const T **out)
{
	void *p = nullptr;
	HIP_OK(hipMalloc(&p, v.size() * sizeof(T)));
	HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
	h->table_allocs.push_back(p);
	*out = (const T *)p;
	return 0;
}

// ---- helpers that cross the files
int ensure_capacity(ofdmrx_handle *h, int n, bool mono, long samples);                    // api_create.cpp
int host_wait(ofdmrx_handle *h);                                                          // api_create.cpp
void run_sc_pass(ofdmrx_handle *h, hipStream_t s, int n, bool force = true, int chunk_seq = 0);   // api_pipeline.cpp
int ensure_events(ofdmrx_handle *h, size_t need);                                           // api_pipeline.cpp: the call's event pool
size_t mark(ofdmrx_handle *h, hipStream_t on = nullptr);                                    // ... one event recorded on `on`
// a call begins: its events and timing spans start over, and it has not been split between two lanes
inline void begin_call(ofdmrx_handle *h)
{
	h->ev_used = 0;
	h->spans.clear();
	h->split_at = 0;
}
int finish_call(ofdmrx_handle *h, int r);                                                   // api_pipeline.cpp: a call ends: r, or the sticky event error
// the chunk pipeline for n records of a stream decode: record k starts from d_records[k] (header, demod, ...); device or pinned
// host outputs like ofdmrx_decode_batch_device; keeps the call's events so far.  fb has stride 0 and, as samples_per_frame, the
// longest source; what record k reads is srcs:
// the records of one or several recordings in one chunk plan - record k reads recording src_of[k], src_len[..] sample frames at
// fb.samples + src_of[k] * stride_bytes (device arrays)
// org (nullable; then src_len and stride_bytes are unused): the sources are live channels read through their windows - position 0 of
// channel q would lie at fb.samples + org[q] bytes and the channel has len[q] sample frames so far (kernels.h: WindowBatch)
struct RecordSources { const int *src_of; const int *src_len; size_t stride_bytes; const long long *org = nullptr; const long long *len = nullptr; };
int decode_records(ofdmrx_handle *h, FrameBatch fb, const SyncState *d_records, size_t n, Outputs out, const RecordSources &srcs);
// p / q -> lowest terms (OFDMRX_E_ARG unless p, q > 0); rechannelize_ratio: and the reduced q <= 16 and 2 <= p / q <= 32
int reduce_ratio(int &p, int &q);                                                           // api_channelize.cpp
int rechannelize_ratio(int &p, int &q);
// the roots of a grid table: dst[2 j], dst[2 j + 1] = e^{+-i pi j / p}, j = 0 .. n - 1 (negative: the minus sign), made in double and
// rounded once
void grid_roots(int p, int n, bool negative, float *dst);
// channelize_centres: OFDMRX_E_ARG for a centre that is not finite or outside +- Rw / 2 - real (a real capture): or
// with |f| < rate / 4 or |f| > Rw / 2 - rate / 4; channelize_setup checks the same and sets the device tables up
int channelize_centres(int rate, int p, int q, const double *centre_hz, size_t n_channels, bool real);
int channelize_setup(ofdmrx_handle *h, int p, int q, const double *centre_hz, size_t n_channels, bool real = false);   // (p / q reduced; q = 1: decimation p)
// the grid front end: decim a power of two 2 .. 512 (else OFDMRX_E_ARG); the slots of a grid table, -decim ..
// decim - 1 each (slots = nullptr: all 2 decim in ascending order, n_slots must be 2 decim), and the table itself on the device
int channelize_grid_decim(int decim);
int channelize_grid_slots(int decim, const int32_t *slots, size_t n_slots, std::vector<int32_t> &out);
int channelize_grid_setup(ofdmrx_handle *h, int decim, const std::vector<int32_t> &slots);
// the grid front end at a ratio: the reduced p / q (else OFDMRX_E_ARG), its slots, its table - 4.19's where q = 1 and
// p is a power of two; launch_channelize_any: the kernel the table set up last belongs to
int channelize_grid_ratio(int &p, int &q);
void channelize_grid_ratio_range(int p, int q, int32_t &k_first, size_t &n_all);
int channelize_grid_ratio_slots(int p, int q, const int32_t *slots, size_t n_slots, std::vector<int32_t> &out);
int channelize_grid_ratio_setup(ofdmrx_handle *h, int p, int q, const std::vector<int32_t> &slots);
void launch_channelize_any(hipStream_t s, const ChannelizeArgs &a);
// the ChannelizeArgs fields the device tables give: taps, inc, grid, tw (the table set up last)
void channelize_tables(const ofdmrx_handle *h, ChannelizeArgs &a);
void bank_free(ofdmrx_handle *h);                                                           // api_bank.cpp: the open bank (or feed) and its windows go
