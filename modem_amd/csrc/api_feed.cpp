// api_feed.cpp -- ofdmrx_feed_*: a recording decoded block by block as it arrives.
//   push: the new samples join a WINDOW of the stream in device memory (raw samples; mono input: the DC blocker's kept states and
//   the analytic signal as well) | the stream scan of api_stream.cpp over the tiles the push has completed, from the trigger carry
//   the last push left | the header stage for preambles whose header symbol has arrived (their mode says when their frame is
//   complete) | the records that are due through the chunk pipeline (decode_records), in preamble order | delivery
//   end:  the last partial tile with n = the samples fed, every pending preamble, delivery
// Every kernel sees absolute stream positions: the views below hand it the address position 0 WOULD have (the window's buffer
// minus its base) and n = the samples fed, so a position past the end reads as zero as in a one-call decode; positions below the
// base are not in memory, and every launch is preceded by a check that it reads none of them (covers()).
#include "api_internal.h"
#include <deque>

struct FeedPending { SyncState st; int mode; };               // mode: -1 header not looked at yet, 0 header failed, else 6 .. 13
struct FeedReady { std::vector<uint8_t> payload; Result res; std::vector<float> rows; };

struct ofdmrx_feed {
	int fmt = 0, channels = 2;
	long long fed = 0;                                        // samples pushed so far
	long long base = 0;                                       // first position the window holds: a multiple of STREAM_TILE
	long long scanned = 0;                                    // the scan's frontier: a multiple of STREAM_TILE until end()
	long long cap = 0;                                        // samples the window's buffers hold
	int cur = 0;                                              // which buffer of each pair is the window (the other one: where it moves to)
	DevBuf raw[2], z[2], ck[2];
	DevBuf dc_end, dc_in, carry, seeds;
	int carry_cur = 0;                                        // carry[carry_cur]: what enters the next push's first tile
	StreamCarry carry_h{ 0, -INFINITY, -1, 0 };               // ... on the host
	long long n_edges = 0, n_acc = 0;                         // falling edges / accepted preambles so far
	long long ck_done = 0;                                    // mono: the DC blocker's states are kept for the blocks below it (a multiple of 64)
	long long z_done = 0;                                     // mono: the analytic signal is formed below it
	std::deque<FeedPending> pend;                             // accepted, not decoded yet (stream order)
	std::deque<FeedReady> ready;                              // decoded, not delivered yet
	bool ending = false;
};

void feed_free(ofdmrx_handle *h)
{
	delete h->feed;
	h->feed = nullptr;
}

namespace {

constexpr long MONO_CK_LEN = 64;                              // samples per kept state of the DC blocker (mono_front.h: MONO_CK)
struct Lens { long sl, stride, buffer_len, ml, md; };
Lens lens_of(int rate)
{
	RX_RATE_SWITCH(rate, return (Lens{ RateCfg<RATE>::SL, RateCfg<RATE>::STRIDE, RateCfg<RATE>::BUFFER_LEN, RateCfg<RATE>::MATCH_LEN, RateCfg<RATE>::MATCH_DEL }));
	return Lens{};
}
size_t frame_bytes(const ofdmrx_feed &f) { return sample_bytes(f.fmt) * (size_t)f.channels; }
const void *origin_of(const DevBuf &b, long long base, size_t unit)   // the address position 0 would have
{
	return (const void *)((uintptr_t)b.p - (uintptr_t)base * unit);
}
// what the scan and the record pipeline read: I/Q pairs at absolute positions (mono input: the analytic signal)
FrameBatch view_iq(const ofdmrx_feed &f)
{
	if (f.channels == 1)
		return FrameBatch{ origin_of(f.z[f.cur], f.base, sizeof(cf)), 0, (long)f.fed, OFDMRX_FMT_F32, 2 };
	return FrameBatch{ origin_of(f.raw[f.cur], f.base, frame_bytes(f)), 0, (long)f.fed, f.fmt, 2 };
}
// a launch reads no position below `lo`: the window must begin at or before it (positions below 0 and from `fed` on read as zero)
int covers(const ofdmrx_feed &f, long long lo, const char *what)
{
	if (std::max(lo, 0LL) >= f.base && f.fed - f.base <= f.cap)
		return 0;
	g_last_error = std::string("feed: the window does not cover what ") + what + " reads";
	return OFDMRX_E_ARG;
}

// How far the window's base may advance: nothing that still looks back reaches below it.
//   the scan and the accept step of the next tiles: BUFFER_LEN behind the frontier (the accept window of an edge at the frontier
//   begins BUFFER_LEN - 1 before it; the tile sums reach MATCH_LEN + 4 STRIDE - 2, direct_P of a maximum at the frontier MATCH_DEL + 4 STRIDE - 2)
//   while the trigger is on: direct_P of the run's maximum so far (the next edge's maximum is that one or a later one; while the
//   trigger is off every value since the last edge is at most `hi`, so the next run's maximum lies at or behind the frontier)
//   the oldest preamble not yet decoded: its Schmidl-Cox body (the header and the demodulator read from sc_start + STRIDE on)
//   mono input: the front end recomputes the stretch the last push ended in from its kept state (at most 256 + 64 samples before it)
long long next_base(const ofdmrx_handle *h)
{
	const ofdmrx_feed &f = *h->feed;
	const Lens L = lens_of(h->rate);
	long long lim = f.scanned - L.buffer_len;
	if (f.carry_h.s == 1 && f.carry_h.i >= 0)
		lim = std::min(lim, f.carry_h.i - (L.md + 4 * L.stride));
	if (!f.pend.empty())
		lim = std::min(lim, (long long)f.pend.front().st.sc_start);
	if (f.channels == 1)
		lim = std::min(lim, f.z_done / front_end_stretch() * front_end_stretch() - 320);
	lim = std::max(lim, 0LL);
	return std::max(lim / STREAM_TILE * STREAM_TILE, f.base);
}

// the window moves to base nb and gets room for `need` samples: what is kept goes to the other buffer of each pair
int move_window(ofdmrx_handle *h, long long nb, long long need)
{
	ofdmrx_feed &f = *h->feed;
	if (nb == f.base && need <= f.cap)
		return 0;
	long long ncap = f.cap;
	if (need > ncap)
		ncap = (need + need / 2 + STREAM_TILE - 1) / STREAM_TILE * STREAM_TILE;
	const int o = f.cur ^ 1;
	const size_t fbytes = frame_bytes(f);
	const long long keep = f.fed - nb, off = nb - f.base;
	int r = f.raw[o].ensure((size_t)ncap * fbytes);
	if (f.channels == 1) {
		r = r ? r : f.z[o].ensure((size_t)ncap * sizeof(cf));
		r = r ? r : f.ck[o].ensure((size_t)(ncap / MONO_CK_LEN + 2) * sizeof(double));
	}
	if (r)
		return r;
	if (keep > 0) {
		HIP_OK(hipMemcpyAsync(f.raw[o].p, (const char *)f.raw[f.cur].p + (size_t)off * fbytes, (size_t)keep * fbytes, hipMemcpyDeviceToDevice, h->stream));
		if (f.channels == 1) {
			HIP_OK(hipMemcpyAsync(f.z[o].p, (const char *)f.z[f.cur].p + (size_t)off * sizeof(cf), (size_t)keep * sizeof(cf), hipMemcpyDeviceToDevice, h->stream));
			const long long blocks = (f.ck_done - nb) / MONO_CK_LEN;
			if (blocks > 0)
				HIP_OK(hipMemcpyAsync(f.ck[o].p, (const char *)f.ck[f.cur].p + (size_t)(off / MONO_CK_LEN) * sizeof(double), (size_t)blocks * sizeof(double),
					hipMemcpyDeviceToDevice, h->stream));
		}
	}
	f.cur = o;
	f.base = nb;
	f.cap = ncap;
	return 0;
}

// mono input: the DC blocker's states of the blocks the push completed, then the analytic signal of the new samples (the stretch the
// last push ended in is formed again from its start: the same values, and its new samples with them)
int front_end(ofdmrx_handle *h)
{
	ofdmrx_feed &f = *h->feed;
	hipStream_t s = h->stream;
	if (f.z_done == f.fed)
		return 0;
	const FrameBatch fb{ origin_of(f.raw[f.cur], f.base, frame_bytes(f)), 0, (long)f.fed, f.fmt, 1 };
	double *ck = (double *)origin_of(f.ck[f.cur], f.base / MONO_CK_LEN, sizeof(double));
	const long long ck_new = f.fed / MONO_CK_LEN * MONO_CK_LEN;
	if (ck_new > f.ck_done) {
		int r = covers(f, f.ck_done - MONO_CK_LEN, "the DC blocker");
		const long ntiles = (long)((f.fed - f.ck_done + 4095) / 4096);
		r = r ? r : f.dc_end.ensure((size_t)ntiles * sizeof(double));
		r = r ? r : f.dc_in.ensure((size_t)ntiles * sizeof(double));
		if (r)
			return r;
		launch_stream_dc_window(s, fb, h->host.front, f.dc_end.as<double>(), f.dc_in.as<double>(), ck, (long)f.ck_done);
		f.ck_done = ck_new;
	}
	const long FE = front_end_stretch();
	const long long s0 = f.z_done / FE, s1 = (f.fed + FE - 1) / FE;
	int r = covers(f, s0 * FE - 320, "the front end");
	if (r)
		return r;
	launch_front_end_window(s, h->rate, fb, mono_args(h->host.front, ck, 0), (cf *)origin_of(f.z[f.cur], f.base, sizeof(cf)), (long)s0, (long)(s1 - s0));
	HIP_OK(hipGetLastError());
	f.z_done = f.fed;
	return 0;
}

// the stream scan over the tiles that are complete (last: every tile that holds a sample), from the carry of the last push;
// the SyncStates of the preambles it accepts join `pend`
int scan(ofdmrx_handle *h, bool last)
{
	ofdmrx_feed &f = *h->feed;
	hipStream_t s = h->stream;
	const Lens L = lens_of(h->rate);
	const long long tile0 = f.scanned / STREAM_TILE, t_end = last ? (f.fed + STREAM_TILE - 1) / STREAM_TILE : f.fed / STREAM_TILE;
	const long ntiles = (long)(t_end - tile0);
	if (ntiles <= 0) {
		if (last)
			f.scanned = std::max(f.scanned, f.fed);
		return 0;
	}
	// the lowest position the tiles, the accept step and direct_P read (see next_base)
	long long lo = f.scanned - (L.buffer_len - 1);
	if (f.carry_h.s == 1 && f.carry_h.i >= 0)
		lo = std::min(lo, f.carry_h.i - (L.md + 4 * L.stride - 2));
	int r = covers(f, lo, "the scan");
	if (r)
		return r;
	if (h->sx_edge_cap == 0)
		h->sx_edge_cap = 4096;
	const FrameBatch fb2 = view_iq(f);
	r = h->sx_counts.ensure(4 * sizeof(long long));
	r = r ? r : h->sx_fn.ensure((size_t)ntiles * sizeof(StreamFn));
	r = r ? r : h->sx_carry.ensure((size_t)ntiles * sizeof(StreamCarry));
	if (r)
		return r;
	StreamCarry *c_in = f.carry.as<StreamCarry>() + f.carry_cur, *c_out = f.carry.as<StreamCarry>() + (f.carry_cur ^ 1);
	long long counts[3] = { 0, 0, 0 };
	StreamCarry out{};
	for (int pass = 0; pass < 2; ++pass) {
		const long cap = h->sx_edge_cap;
		r = h->sx_edges.ensure((size_t)cap * sizeof(StreamEdge));
		r = r ? r : h->sx_rec.ensure((size_t)cap * sizeof(SyncState));
		if (r)
			return r;
		HIP_OK(hipMemsetAsync(h->sx_counts.p, 0, 4 * sizeof(long long), s));
		launch_stream_scan_window(s, h->rate, fb2, (long)f.fed, tile0, ntiles, h->sx_fn.as<StreamFn>(), h->sx_carry.as<StreamCarry>(), c_in, c_out,
			h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
		launch_stream_accept_window(s, h->rate, fb2, h->dev, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>(), f.base);
		launch_stream_records(s, h->rate, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>(), h->sx_rec.as<SyncState>(), cap, f.n_acc,
			f.n_edges - f.n_acc);
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemcpyAsync(counts, h->sx_counts.p, sizeof(counts), hipMemcpyDeviceToHost, s));
		HIP_OK(hipMemcpyAsync(&out, c_out, sizeof(out), hipMemcpyDeviceToHost, s));
		HIP_OK(hipStreamSynchronize(s));
		if (counts[0] <= cap)
			break;
		h->sx_edge_cap = (long)counts[0];                         // more falling edges than the buffer held: once more with room for all
	}
	if (counts[2]) {
		g_last_error = "feed: an edge of the scan reads below the window";
		return OFDMRX_E_ARG;
	}
	if (counts[1] > 0) {
		std::vector<SyncState> rec((size_t)counts[1]);
		HIP_OK(hipMemcpy(rec.data(), h->sx_rec.p, rec.size() * sizeof(SyncState), hipMemcpyDeviceToHost));
		for (const SyncState &st : rec)
			f.pend.push_back(FeedPending{ st, -1 });
	}
	f.n_edges += counts[0];
	f.n_acc += counts[1];
	f.carry_h = out;
	f.carry_cur ^= 1;
	f.scanned = last ? f.fed : t_end * STREAM_TILE;
	return 0;
}

// the header stage for the pending preambles whose header symbol has arrived: their mode tells when their frame is complete
int headers(ofdmrx_handle *h)
{
	ofdmrx_feed &f = *h->feed;
	hipStream_t s = h->stream;
	const Lens L = lens_of(h->rate);
	std::vector<size_t> idx;
	for (size_t i = 0; i < f.pend.size(); ++i)
		if (f.pend[i].mode < 0 && f.fed >= (long long)f.pend[i].st.sc_start + L.stride + L.sl)
			idx.push_back(i);
	const FrameBatch fb2 = view_iq(f);
	for (size_t i0 = 0; i0 < idx.size(); i0 += (size_t)h->chunk) {
		const int n = (int)std::min<size_t>((size_t)h->chunk, idx.size() - i0);
		std::vector<SyncState> st((size_t)n);
		for (int k = 0; k < n; ++k)
			st[(size_t)k] = f.pend[idx[i0 + (size_t)k]].st;
		int r = covers(f, (long long)st[0].sc_start + L.stride, "the header stage");
		r = r ? r : ensure_capacity(h, n, false, 0);
		if (r)
			return r;
		HIP_OK(hipMemcpyAsync(h->st.p, st.data(), st.size() * sizeof(SyncState), hipMemcpyHostToDevice, s));
		launch_header(s, h->rate, n, fb2, nullptr, mono_args(h->host.front, nullptr, 0), h->dev, h->st.as<SyncState>(), h->hdr_soft.as<int8_t>(), nullptr, nullptr);
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemcpyAsync(st.data(), h->st.p, st.size() * sizeof(SyncState), hipMemcpyDeviceToHost, s));
		HIP_OK(hipStreamSynchronize(s));
		for (int k = 0; k < n; ++k)
			f.pend[idx[i0 + (size_t)k]].mode = st[(size_t)k].okay ? st[(size_t)k].oper_mode : 0;
	}
	return 0;
}

// the records that are due, in preamble order, through the chunk pipeline; all: every pending one (end of the stream)
int decode_due(ofdmrx_handle *h, bool all)
{
	ofdmrx_feed &f = *h->feed;
	hipStream_t s = h->stream;
	const Lens L = lens_of(h->rate);
	size_t n = 0;
	for (; n < f.pend.size(); ++n) {
		const FeedPending &p = f.pend[n];
		if (all || p.mode == 0)
			continue;
		// the demodulator's last symbol ends at sc_start + (rows + 2) STRIDE + SL: the last sample of the frame
		if (p.mode < 0 || f.fed < (long long)p.st.sc_start + (long long)(mode_desc(p.mode).rows + 2) * L.stride + L.sl)
			break;
	}
	if (n == 0)
		return 0;
	std::vector<SyncState> st(n);
	for (size_t k = 0; k < n; ++k)
		st[k] = f.pend[k].st;
	float *const rows_user = h->esn0_user;
	int r = covers(f, (long long)st[0].sc_start + L.stride, "the record pipeline");
	r = r ? r : f.seeds.ensure(n * sizeof(SyncState));
	r = r ? r : h->sx_pay.ensure(n * PAYLOAD_BYTES);
	r = r ? r : h->sx_res.ensure(n * sizeof(Result));
	if (rows_user)
		r = r ? r : h->sx_esn0.ensure(n * ROWS_MAX * sizeof(float));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(f.seeds.p, st.data(), n * sizeof(SyncState), hipMemcpyHostToDevice, s));
	begin_call(h);
	r = ensure_events(h, 16);
	r = r ? r : decode_records(h, view_iq(f), f.seeds.as<SyncState>(), n, Outputs{ h->sx_pay.as<uint8_t>(), h->sx_res.as<Result>(), rows_user ? h->sx_esn0.as<float>() : nullptr });
	if (r)
		return r;
	std::vector<uint8_t> pay(n * PAYLOAD_BYTES);
	std::vector<Result> res(n);
	std::vector<float> rows(rows_user ? n * ROWS_MAX : 0);
	HIP_OK(hipMemcpyAsync(pay.data(), h->sx_pay.p, pay.size(), hipMemcpyDeviceToHost, s));
	HIP_OK(hipMemcpyAsync(res.data(), h->sx_res.p, n * sizeof(Result), hipMemcpyDeviceToHost, s));
	if (rows_user)
		HIP_OK(hipMemcpyAsync(rows.data(), h->sx_esn0.p, rows.size() * sizeof(float), hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
	for (size_t k = 0; k < n; ++k) {
		FeedReady q;
		q.payload.assign(pay.begin() + (long)(k * PAYLOAD_BYTES), pay.begin() + (long)((k + 1) * PAYLOAD_BYTES));
		q.res = res[k];
		if (rows_user)
			q.rows.assign(rows.begin() + (long)(k * ROWS_MAX), rows.begin() + (long)((k + 1) * ROWS_MAX));
		f.ready.push_back(std::move(q));
		f.pend.pop_front();
	}
	return 0;
}

// the first max_frames staged records leave; the rest wait, in order
void deliver(ofdmrx_handle *h, size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_records, size_t *n_left)
{
	ofdmrx_feed &f = *h->feed;
	size_t k = 0;
	for (; k < max_frames && !f.ready.empty(); ++k) {
		const FeedReady &q = f.ready.front();
		std::memcpy(payload_out + k * PAYLOAD_BYTES, q.payload.data(), PAYLOAD_BYTES);
		std::memcpy(results + k, &q.res, sizeof(Result));
		if (h->esn0_user) {
			if (q.rows.size() == ROWS_MAX)
				std::memcpy(h->esn0_user + k * ROWS_MAX, q.rows.data(), ROWS_MAX * sizeof(float));
			else                                                      // (decoded while the rows were off)
				std::memset(h->esn0_user + k * ROWS_MAX, 0, ROWS_MAX * sizeof(float));
		}
		f.ready.pop_front();
	}
	*n_records = k;
	*n_left = f.ready.size();
}

// one slice of a push: at most PUSH_SLICE samples join the window and are worked through
constexpr size_t PUSH_SLICE = (size_t)1 << 26;
int push_slice(ofdmrx_handle *h, const void *samples, size_t n)
{
	ofdmrx_feed &f = *h->feed;
	int r = move_window(h, next_base(h), f.fed + (long long)n - next_base(h));
	if (r)
		return r;
	if (n) {
		const size_t fbytes = frame_bytes(f);
		HIP_OK(hipMemcpyAsync((char *)f.raw[f.cur].p + (size_t)(f.fed - f.base) * fbytes, samples, n * fbytes, hipMemcpyHostToDevice, h->stream));
		f.fed += (long long)n;
	}
	if (f.channels == 1)
		r = front_end(h);
	r = r ? r : scan(h, false);
	r = r ? r : headers(h);
	r = r ? r : decode_due(h, false);
	if (!r)
		HIP_OK(hipStreamSynchronize(h->stream));                  // (the caller's samples have left)
	return r;
}

int out_args(const ofdmrx_handle *h, size_t max_frames, const void *payload, const void *results, const size_t *n_records, const size_t *n_left)
{
	if (!h || !n_records || !n_left || (max_frames && (!payload || !results)))
		return OFDMRX_E_ARG;
	return 0;
}

}  // namespace

extern "C" int ofdmrx_feed_begin(ofdmrx_handle *h, int fmt, int channels)
{
	if (!h || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || channels < 1 || channels > 2)
		return OFDMRX_E_ARG;
	if (h->feed || h->bank)
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	ofdmrx_feed *f = new (std::nothrow) ofdmrx_feed;
	if (!f)
		return OFDMRX_E_NOMEM;
	f->fmt = fmt;
	f->channels = channels;
	int r = f->carry.ensure(2 * sizeof(StreamCarry));
	if (!r && hipMemcpy(f->carry.p, &f->carry_h, sizeof(StreamCarry), hipMemcpyHostToDevice) != hipSuccess)
		r = OFDMRX_E_HIP;
	if (r) {
		delete f;
		return r;
	}
	h->feed = f;
	return 0;
}

extern "C" int ofdmrx_feed_push(ofdmrx_handle *h, const void *samples, size_t n_samples, size_t max_frames, uint8_t *payload_out,
	ofdmrx_frame_result *results, size_t *n_records, size_t *n_left)
{
	int r = out_args(h, max_frames, payload_out, results, n_records, n_left);
	if (r || (n_samples && !samples))
		return OFDMRX_E_ARG;
	if (!h->feed || (h->feed->ending && n_samples))
		return OFDMRX_E_ARG;
	ofdmrx_feed &f = *h->feed;
	if (n_samples && (size_t)samples % frame_bytes(f))
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	if (!f.ending) {
		size_t done = 0;
		do {                                                      // (a zero-length push still takes what has become due)
			const size_t n = std::min(PUSH_SLICE, n_samples - done);
			r = push_slice(h, (const char *)samples + done * frame_bytes(f), n);
			if (r)
				return r;
			done += n;
		} while (done < n_samples);
	}
	deliver(h, max_frames, payload_out, results, n_records, n_left);
	return 0;
}

extern "C" int ofdmrx_feed_end(ofdmrx_handle *h, size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_records,
	size_t *n_left)
{
	int r = out_args(h, max_frames, payload_out, results, n_records, n_left);
	if (r)
		return r;
	if (!h->feed)
		return OFDMRX_E_ARG;
	ofdmrx_feed &f = *h->feed;
	HIP_OK(hipSetDevice(h->cfg.device));
	if (!f.ending) {
		r = scan(h, true);
		r = r ? r : decode_due(h, true);
		if (r)
			return r;
		HIP_OK(hipStreamSynchronize(h->stream));
		f.ending = true;
	}
	deliver(h, max_frames, payload_out, results, n_records, n_left);
	if (*n_left == 0)
		feed_free(h);
	return 0;
}

// Every kernel of the record pipeline reads inside the frame (the demodulator's last symbol ends on its last sample): no lag
extern "C" long long ofdmrx_feed_lag(ofdmrx_handle *h) { return (h && h->feed) ? 0 : OFDMRX_E_ARG; }

extern "C" long long ofdmrx_feed_resident_samples(ofdmrx_handle *h)
{
	return (h && h->feed) ? h->feed->fed - h->feed->base : OFDMRX_E_ARG;
}
