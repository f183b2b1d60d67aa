// api_bank.cpp -- the live entries: ofdmrx_bank_*, many live channels pushed and decoded in one call, and
// ofdmrx_feed_*, one recording decoded block by block as it arrives: a bank of one channel, at the end of this file.
//   push: the new samples join every channel's WINDOW of its stream in device memory (raw samples; mono input: the DC blocker's kept
//   states and the analytic signal as well), and every stage runs ONCE for all channels:
//   window move (one kernel) | the new samples (packed on the host, one copy, one kernel that places every channel's share in its
//   window) | one scan, accept and records pass over every tile any channel completed (the WindowBatch forms of k_stream.hip with
//   the channel as the second grid dimension, a segmented scan from the trigger carry every channel's last push left) | one
//   read-back of all counts and carries | one header pass over every pending preamble whose header symbol has arrived (its mode says
//   when its frame is complete) | ONE decode_records call over every record that is due on any channel, in channel then preamble
//   order: the records of many channels share chunks | delivery
//   end:  the last partial tile of every channel with n = the samples fed, every pending preamble, delivery
// A WIDEBAND bank (ofdmrx_bank_begin_wideband) is fed one wideband capture instead: its channels are 2-channel F32 at
// the handle's rate, and "the new samples" of a push are made on the device - the wideband block is copied once behind the last
// T - 1 wideband samples (kept on the host and sent with it), and ONE k_channelize launch writes every channel's new samples straight
// into its window (a bank opened with ofdmrx_bank_begin_wideband_ratio, DESIGN.md 4.17: ONE k_rechannelize launch; with
// ofdmrx_bank_begin_wideband_grid, DESIGN.md 4.19: ONE k_channelize_grid launch, the tail up to 24 x 512 samples; with
// ofdmrx_bank_begin_wideband_real, DESIGN.md 4.25: a REAL capture, one value per wideband sample frame, ONE launch of the same
// k_channelize or k_rechannelize instantiated for it).  Everything behind
// that step is the same code.
// The windows of all channels live in one slab pair [n_channels][cap] with a common capacity; channel c's window begins at its own
// base[c].  Every kernel sees absolute positions of the channel it reads (kernels.h: WindowBatch: it is handed the address position 0
// WOULD have and n = the samples fed, so a position past the end reads as zero as in a one-call decode); positions below the base are
// not in memory, and before any launch the host checks, for every channel the launch touches, that the channel's window holds every
// position the launch reads (covers()).
#include "api_internal.h"
#include <deque>

struct BankPending { SyncState st; int mode; long long index; };    // mode: -1 header not looked at yet, 0 header failed, else 6 .. 13
struct BankReady { std::vector<uint8_t> payload; Result res; std::vector<float> rows; int32_t channel; int64_t index; };
struct BankChannel {
	long long fed = 0;                                        // samples pushed so far
	long long base = 0;                                       // first position the window holds: a multiple of STREAM_TILE
	long long scanned = 0;                                    // the scan's frontier: a multiple of STREAM_TILE until the channel ends
	StreamCarry carry{ 0, -INFINITY, -1, 0 };                 // what enters the channel's next tile (host copy)
	long long n_edges = 0, n_acc = 0;                         // falling edges / accepted preambles so far
	long long ck_done = 0;                                    // mono: the DC blocker's states are kept for the blocks below it (a multiple of 64)
	long long z_done = 0;                                     // mono: the analytic signal is formed below it
	std::deque<BankPending> pend;                             // accepted, not decoded yet (stream order)
	bool ended = false;
};

struct ofdmrx_bank {
	int fmt = 0, channels = 2;
	size_t C = 0;
	long long cap = 0;                                        // samples every channel's window can hold
	int cur = 0;                                              // which slab of the pair holds the windows
	DevBuf raw[2], z[2], ck[2];                               // [C][cap] sample frames; mono: [C][cap] cf, [C][cap / 64 + 2] doubles
	DevBuf dc_end, dc_in;
	DevBuf par, stage, carry, seeds, seed_src, hdr_src;
	int carry_cur = 0;
	long edge_cap = 0, rec_cap = 0;                           // every channel's share of the edge buffer; records one push may bring
	std::vector<BankChannel> ch;
	std::deque<BankReady> ready;                              // decoded, not delivered yet
	std::vector<long long> par_h, counts_h;                   // (host sides of the copies: they live as long as the bank)
	std::vector<StreamCarry> carry_h;
	std::vector<char> stage_h;
	long long ops = 0;                                        // launches + copies + synchronisations of the last call's own stages
	bool ending = false;
	bool as_feed = false;                                     // opened by ofdmrx_feed_begin: the ofdmrx_feed_* entries serve it, ofdmrx_bank_* refuse it
	// a wideband bank: decimation, the format of the wideband samples, how many have been pushed, and the last min(wfed, T - 1) of them
	// (decimation p / q in lowest terms: an integer decimation has q = 1 and runs k_channelize, any other k_rechannelize, DESIGN.md 4.17;
	// a grid bank, DESIGN.md 4.19, has q = 1 and runs k_channelize_grid: the handle's table says so, which the open bank owns)
	// (wreal: a real capture, DESIGN.md 4.25 - one value per wideband position, the same two kernels instantiated for it)
	bool wide = false, wreal = false;
	int p = 0, q = 1, wfmt = 0;
	long long wfed = 0;
	std::vector<char> wtail;
};

void bank_free(ofdmrx_handle *h)
{
	delete h->bank;
	h->bank = nullptr;
}

namespace {

constexpr long MONO_CK_LEN = 64;                              // samples per kept state of the DC blocker (mono_front.h: MONO_CK)
struct Lens { long sl, stride, buffer_len, ml, md; };
Lens lens_of(int rate)
{
	RX_RATE_SWITCH(rate, return (Lens{ RateCfg<RATE>::SL, RateCfg<RATE>::STRIDE, RateCfg<RATE>::BUFFER_LEN, RateCfg<RATE>::MATCH_LEN, RateCfg<RATE>::MATCH_DEL }));
	return Lens{};
}
size_t frame_bytes(const ofdmrx_bank &b) { return sample_bytes(b.fmt) * (size_t)b.channels; }
// a wideband bank: bytes per wideband sample frame - I/Q, or the one value of a real capture
size_t wide_bytes(const ofdmrx_bank &b) { return (b.wreal ? 1 : 2) * sample_bytes(b.wfmt); }

// the per-channel arrays a call uploads in one copy, P = C + 1 values each
// (the window move has three planes: raw samples, analytic signal, DC states; sources and destinations are addresses)
enum { P_MV_SRC, P_MV_DST = P_MV_SRC + 3, P_MV_BYTES = P_MV_DST + 3, P_PL_SRC = P_MV_BYTES + 3, P_PL_DST, P_PL_BYTES, P_ORG, P_LEN, P_LO, P_TILE0,
	P_TILE_AT, P_REC_BASE, P_REJ_BASE, P_BELOW, P_ZORG, P_CKORG, P_DC_FROM, P_DC_AT, P_FE0, P_FE_AT, P_COUNT };

// a launch reads no position of channel c below `lo`: its window must begin at or before it
int covers(const ofdmrx_bank &b, size_t c, long long lo, const char *what)
{
	const BankChannel &k = b.ch[c];
	if (std::max(lo, 0LL) >= k.base && k.fed - k.base <= b.cap)
		return 0;
	g_last_error = std::string("bank: the window of channel ") + std::to_string(c) + " does not cover what " + what + " reads";
	return OFDMRX_E_ARG;
}

// How far the base of a channel's window may advance: nothing that still looks back reaches below it.
//   the scan and the accept step of the next tiles: BUFFER_LEN behind the frontier (the accept window of an edge at the frontier
//   begins BUFFER_LEN - 1 before it; the tile sums reach MATCH_LEN + 4 STRIDE - 2, direct_P of a maximum at the frontier MATCH_DEL + 4 STRIDE - 2)
//   while the trigger is on: direct_P of the run's maximum so far (the next edge's maximum is that one or a later one; while the
//   trigger is off every value since the last edge is at most `hi`, so the next run's maximum lies at or behind the frontier)
//   the oldest preamble not yet decoded: its Schmidl-Cox body (the header and the demodulator read from sc_start + STRIDE on)
//   mono input: the front end recomputes the stretch the last push ended in from its kept state (at most 256 + 64 samples before it)
long long next_base(const BankChannel &k, const Lens &L, bool mono)
{
	long long lim = k.scanned - L.buffer_len;
	if (k.carry.s == 1 && k.carry.i >= 0)
		lim = std::min(lim, k.carry.i - (L.md + 4 * L.stride));
	if (!k.pend.empty())
		lim = std::min(lim, (long long)k.pend.front().st.sc_start);
	if (mono)
		lim = std::min(lim, k.z_done / front_end_stretch() * front_end_stretch() - 320);
	lim = std::max(lim, 0LL);
	return std::max(lim / STREAM_TILE * STREAM_TILE, k.base);
}

// raw: the samples as they arrived (what the mono front end reads); else what the scan and the record pipeline read: I/Q pairs at
// absolute positions (mono input: the analytic signal)
WindowBatch window_batch(const ofdmrx_bank &b, const int *src_of, bool raw = false)
{
	const size_t P = b.C + 1;
	long long *p = b.par.as<long long>();
	const bool mono = b.channels == 1;
	WindowBatch w{};
	w.samples = (mono && !raw) ? b.z[b.cur].p : b.raw[b.cur].p;
	w.frame_stride_bytes = 0;
	w.samples_per_frame = 0;
	w.fmt = (mono && !raw) ? OFDMRX_FMT_F32 : b.fmt;
	w.channels = raw ? b.channels : 2;
	w.src_of = src_of;
	w.org = p + ((mono && !raw) ? P_ZORG : P_ORG) * P;
	w.len = p + P_LEN * P;
	w.lo = p + P_LO * P;
	w.tile0 = p + P_TILE0 * P;
	w.tile_at = p + P_TILE_AT * P;
	w.below = p + P_BELOW * P;
	w.z_org = p + P_ZORG * P;
	w.ck_org = p + P_CKORG * P;
	w.dc_from = p + P_DC_FROM * P;
	w.dc_at = p + P_DC_AT * P;
	w.fe0 = p + P_FE0 * P;
	w.fe_at = p + P_FE_AT * P;
	return w;
}

// One call's work: every channel c takes add[c] more samples (nullable: none), those with fin[c] end behind them.
// A wideband bank: samples are n_wide wideband sample frames, and add[c] is what they give every channel.
int bank_step(ofdmrx_handle *h, const char *samples, size_t stride, const size_t *add, const std::vector<uint8_t> &fin, size_t n_wide = 0)
{
	ofdmrx_bank &b = *h->bank;
	hipStream_t s = h->stream;
	const Lens L = lens_of(h->rate);
	const size_t C = b.C, P = C + 1, unit = frame_bytes(b);
	std::vector<long long> &par = b.par_h;
	par.assign((size_t)P_COUNT * P, 0);
	auto at = [&](int what, size_t c) -> long long & { return par[(size_t)what * P + c]; };

	const bool mono = b.channels == 1;
	const long FE = front_end_stretch();
	auto ck_row = [](long long cap) { return cap / MONO_CK_LEN + 2; };   // kept states per channel
	// ---- 1. every channel's new base; the common capacity
	std::vector<long long> nb(C);
	long long need = 0;
	bool moves = false;
	for (size_t c = 0; c < C; ++c) {
		const BankChannel &k = b.ch[c];
		nb[c] = next_base(k, L, mono);
		moves |= nb[c] != k.base;
		need = std::max(need, k.fed + (long long)(add ? add[c] : 0) - nb[c]);
	}
	long long ncap = b.cap;
	if (need > ncap)
		ncap = (need + need / 2 + STREAM_TILE - 1) / STREAM_TILE * STREAM_TILE;
	moves |= ncap != b.cap;
	const int o = moves ? b.cur ^ 1 : b.cur;                      // where the windows are behind the move
	long long mv_most = 0;
	if (moves) {
		int r = b.raw[o].ensure(C * (size_t)ncap * unit);
		if (mono) {
			r = r ? r : b.z[o].ensure(C * (size_t)ncap * sizeof(cf));
			r = r ? r : b.ck[o].ensure(C * (size_t)ck_row(ncap) * sizeof(double));
		}
		if (r)
			return r;
		for (size_t c = 0; c < C; ++c) {
			const BankChannel &k = b.ch[c];
			const long long off = nb[c] - k.base, keep = k.fed - nb[c];
			// (inside both slabs: the kept range is part of the old window, and no longer than the new capacity)
			if (off < 0 || keep < 0 || k.fed - k.base > b.cap || keep > ncap) {
				g_last_error = "bank: a window move would leave its buffers";
				return OFDMRX_E_ARG;
			}
			if (keep == 0)
				continue;
			at(P_MV_SRC, c) = (long long)(uintptr_t)b.raw[b.cur].p + ((long long)c * b.cap + off) * (long long)unit;
			at(P_MV_DST, c) = (long long)(uintptr_t)b.raw[o].p + (long long)c * ncap * (long long)unit;
			at(P_MV_BYTES, c) = keep * (long long)unit;
			mv_most = std::max(mv_most, at(P_MV_BYTES, c));
			if (mono) {
				at(P_MV_SRC + 1, c) = (long long)(uintptr_t)b.z[b.cur].p + ((long long)c * b.cap + off) * (long long)sizeof(cf);
				at(P_MV_DST + 1, c) = (long long)(uintptr_t)b.z[o].p + (long long)c * ncap * (long long)sizeof(cf);
				at(P_MV_BYTES + 1, c) = keep * (long long)sizeof(cf);
				mv_most = std::max(mv_most, at(P_MV_BYTES + 1, c));
				const long long blocks = (k.ck_done - nb[c]) / MONO_CK_LEN;
				if (blocks > 0) {
					if (blocks > ck_row(ncap) || off / MONO_CK_LEN + blocks > ck_row(b.cap)) {
						g_last_error = "bank: a window move would leave its buffers";
						return OFDMRX_E_ARG;
					}
					at(P_MV_SRC + 2, c) = (long long)(uintptr_t)b.ck[b.cur].p + ((long long)c * ck_row(b.cap) + off / MONO_CK_LEN) * (long long)sizeof(double);
					at(P_MV_DST + 2, c) = (long long)(uintptr_t)b.ck[o].p + (long long)c * ck_row(ncap) * (long long)sizeof(double);
					at(P_MV_BYTES + 2, c) = blocks * (long long)sizeof(double);
				}
			}
		}
	}
	// ---- 2. the new samples, packed so that every share lies as its place in the window does modulo 16
	size_t packed = 0;
	long long pl_most = 0;
	const size_t wunit = wide_bytes(b);
	try {
		size_t total = b.wide ? b.wtail.size() + n_wide * wunit : 0;
		for (size_t c = 0; c < C && add && !b.wide; ++c)
			total += add[c] * unit + 32;
		b.stage_h.resize(total);
	} catch (const std::bad_alloc &) {
		return OFDMRX_E_NOMEM;
	}
	for (size_t c = 0; c < C; ++c) {
		const BankChannel &k = b.ch[c];
		const size_t n = add ? add[c] : 0;
		if (n) {
			if (k.fed + (long long)n - nb[c] > ncap) {
				g_last_error = "bank: new samples would leave their window";
				return OFDMRX_E_ARG;
			}
			const long long dst = (long long)(uintptr_t)b.raw[o].p + ((long long)c * ncap + (k.fed - nb[c])) * (long long)unit;
			if (b.wide) {                                             // k_channelize writes the share there
				at(P_PL_DST, c) = dst;
				continue;
			}
			const size_t src = (packed + 15) / 16 * 16 + (size_t)(dst & 15);
			std::memcpy(b.stage_h.data() + src, samples + c * stride, n * unit);
			at(P_PL_SRC, c) = (long long)src;                         // (the staging buffer's address joins it below)
			at(P_PL_DST, c) = dst;
			at(P_PL_BYTES, c) = (long long)(n * unit);
			pl_most = std::max(pl_most, (long long)(n * unit));
			packed = src + n * unit;
		}
	}
	int r = packed ? b.stage.ensure(packed) : 0;
	if (r)
		return r;
	for (size_t c = 0; c < C; ++c)
		if (at(P_PL_BYTES, c))
			at(P_PL_SRC, c) += (long long)(uintptr_t)b.stage.p;
	// ---- the state behind the move and the new samples: what every kernel of this call sees
	long long total_tiles = 0, max_tiles = 0, dc_tiles = 0, dc_most = 0, fe_total = 0, fe_most = 0;
	std::vector<long long> t_end(C, 0);
	for (size_t c = 0; c < C; ++c) {
		BankChannel &k = b.ch[c];
		k.base = nb[c];
		k.fed += (long long)(add ? add[c] : 0);
		at(P_ORG, c) = ((long long)c * ncap - k.base) * (long long)unit;
		at(P_ZORG, c) = ((long long)c * ncap - k.base) * (long long)sizeof(cf);
		at(P_CKORG, c) = ((long long)c * ck_row(ncap) - k.base / MONO_CK_LEN) * (long long)sizeof(double);
		at(P_LEN, c) = k.fed;
		at(P_LO, c) = k.base;
		long long nt = 0;
		if (!k.ended) {
			const long long tile0 = k.scanned / STREAM_TILE;
			t_end[c] = fin[c] ? (k.fed + STREAM_TILE - 1) / STREAM_TILE : k.fed / STREAM_TILE;
			nt = std::max(0LL, t_end[c] - tile0);
			at(P_TILE0, c) = tile0;
		}
		at(P_TILE_AT, c) = total_tiles;
		total_tiles += nt;
		max_tiles = std::max(max_tiles, nt);
		at(P_REC_BASE, c) = k.n_acc;
		at(P_REJ_BASE, c) = k.n_edges - k.n_acc;
		// mono: the DC blocker's states of the blocks the push completed, then the analytic signal of the new samples (the stretch the
		// last push ended in is formed again from its start: the same values, and its new samples with them)
		long long dct = 0, fen = 0;
		if (mono && k.z_done != k.fed) {
			if (k.fed / MONO_CK_LEN * MONO_CK_LEN > k.ck_done) {
				dct = (k.fed - k.ck_done + 4095) / 4096;
				at(P_DC_FROM, c) = k.ck_done;
			}
			at(P_FE0, c) = k.z_done / FE;
			fen = (k.fed + FE - 1) / FE - k.z_done / FE;
		}
		at(P_DC_AT, c) = dc_tiles;
		dc_tiles += dct;
		dc_most = std::max(dc_most, dct);
		at(P_FE_AT, c) = fe_total;
		fe_total += fen;
		fe_most = std::max(fe_most, fen);
	}
	at(P_TILE_AT, C) = total_tiles;
	at(P_DC_AT, C) = dc_tiles;
	at(P_FE_AT, C) = fe_total;
	r = b.par.ensure(par.size() * sizeof(long long));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(b.par.p, par.data(), par.size() * sizeof(long long), hipMemcpyHostToDevice, s));
	b.ops += 1;
	long long *dpar = b.par.as<long long>();
	if (moves) {
		if (mv_most > 0) {
			launch_bank_copy(s, (int)C, mono ? 3 : 1, P, mv_most, dpar + P_MV_SRC * P, dpar + P_MV_DST * P, dpar + P_MV_BYTES * P);
			b.ops += 1;
		}
		b.cur = o;
		b.cap = ncap;
	}
	if (packed) {
		HIP_OK(hipMemcpyAsync(b.stage.p, b.stage_h.data(), packed, hipMemcpyHostToDevice, s));
		launch_bank_copy(s, (int)C, 1, P, pl_most, dpar + P_PL_SRC * P, dpar + P_PL_DST * P, dpar + P_PL_BYTES * P);
		b.ops += 2;
	}
	if (b.wide && n_wide) {
		// the block behind the kept tail, one copy; one launch for every channel's new outputs ceil(W_old / D) .. ceil(W_new / D) - 1.
		// The first of them reads from ceil(W_old / D) D - (T - 1) >= W_old - (T - 1) on: inside the tail, or below position 0
		// (D = p / q: output n >= ceil(W_old q / p) reads from n p div q - (T - 1) >= W_old - (T - 1) on)
		const long long num = b.p, den = b.q, T = 24 * num / den + 1, tail = (long long)(b.wtail.size() / wunit);
		const long long o0 = (b.wfed * den + num - 1) / num, o1 = ((b.wfed + (long long)n_wide) * den + num - 1) / num;
		std::memcpy(b.stage_h.data(), b.wtail.data(), b.wtail.size());
		std::memcpy(b.stage_h.data() + b.wtail.size(), samples, n_wide * wunit);
		if (o1 > o0) {
			if ((size_t)(o1 - o0) != (add ? add[0] : 0) || (tail < T - 1 && tail != b.wfed)) {
				g_last_error = "bank: the wideband tail does not hold what the new outputs read";
				return OFDMRX_E_ARG;
			}
			r = b.stage.ensure(b.stage_h.size());
			if (r)
				return r;
			HIP_OK(hipMemcpyAsync(b.stage.p, b.stage_h.data(), b.stage_h.size(), hipMemcpyHostToDevice, s));
			ChannelizeArgs a{};
			a.in = b.stage.p;
			a.fmt = b.wfmt;
			a.p = b.p;
			a.q = b.q;
			a.in_first = b.wfed - tail;
			a.n_in = tail + (long long)n_wide;
			channelize_tables(h, a);
			a.n_channels = (int)C;
			a.out_first = o0;
			a.n_out = o1 - o0;
			a.dst = dpar + P_PL_DST * P;
			a.real = b.wreal;
			launch_channelize_any(s, a);
			b.ops += 2;
		}
		const size_t keep = std::min(b.stage_h.size(), (size_t)(T - 1) * wunit);
		b.wtail.assign(b.stage_h.end() - (long)keep, b.stage_h.end());
		b.wfed += (long long)n_wide;
	}
	HIP_OK(hipGetLastError());
	// ---- 3. mono input: every channel's DC-blocker states and analytic signal, each composed from that channel's own positions alone
	if (fe_total > 0) {
		for (size_t c = 0; c < C; ++c) {
			const BankChannel &k = b.ch[c];
			if (at(P_DC_AT, c + 1) > at(P_DC_AT, c) && (r = covers(b, c, k.ck_done - MONO_CK_LEN, "the DC blocker")))
				return r;
			if (at(P_FE_AT, c + 1) > at(P_FE_AT, c) && (r = covers(b, c, at(P_FE0, c) * FE - 320, "the front end")))
				return r;
		}
		const WindowBatch wr = window_batch(b, nullptr, true);
		if (dc_tiles > 0) {
			r = b.dc_end.ensure((size_t)dc_tiles * sizeof(double));
			r = r ? r : b.dc_in.ensure((size_t)dc_tiles * sizeof(double));
			if (r)
				return r;
			launch_bank_dc(s, (int)C, (long)dc_most, wr, h->host.front, b.dc_end.as<double>(), b.dc_in.as<double>(), b.ck[b.cur].as<double>());
			b.ops += 3;
		}
		launch_bank_front_end(s, h->rate, (int)C, (long)fe_most, wr, mono_args(h->host.front, b.ck[b.cur].as<double>(), 0), b.z[b.cur].as<cf>());
		b.ops += 1;
		HIP_OK(hipGetLastError());
		for (size_t c = 0; c < C; ++c) {
			BankChannel &k = b.ch[c];
			k.ck_done = std::max(k.ck_done, k.fed / MONO_CK_LEN * MONO_CK_LEN);
			k.z_done = k.fed;
		}
	}

	// ---- 4. / 5. one scan, accept and records pass over every tile any channel completed; one read-back
	if (total_tiles > 0) {
		for (size_t c = 0; c < C; ++c) {
			const BankChannel &k = b.ch[c];
			if (at(P_TILE_AT, c + 1) == at(P_TILE_AT, c))
				continue;
			// the lowest position the tiles, the accept step and direct_P read (see next_base)
			long long lo = k.scanned - (L.buffer_len - 1);
			if (k.carry.s == 1 && k.carry.i >= 0)
				lo = std::min(lo, k.carry.i - (L.md + 4 * L.stride - 2));
			if ((r = covers(b, c, lo, "the scan")))
				return r;
		}
		if (b.edge_cap == 0)
			b.edge_cap = std::max(256L, std::min(4096L, (long)((64u << 20) / sizeof(StreamEdge) / C)));
		if (b.rec_cap == 0)
			b.rec_cap = (long)std::max<size_t>(4096, 4 * C);
		const WindowBatch wb = window_batch(b, nullptr);
		r = h->sx_counts.ensure(2 * C * sizeof(long long));
		r = r ? r : h->sx_fn.ensure((size_t)total_tiles * sizeof(StreamFn));
		r = r ? r : h->sx_carry.ensure((size_t)total_tiles * sizeof(StreamCarry));
		r = r ? r : h->sxs_first.ensure(P * sizeof(long long));
		if (r)
			return r;
		StreamCarry *c_in = b.carry.as<StreamCarry>() + (size_t)b.carry_cur * C, *c_out = b.carry.as<StreamCarry>() + (size_t)(b.carry_cur ^ 1) * C;
		std::vector<long long> &counts = b.counts_h;
		counts.assign(3 * C, 0);
		b.carry_h.resize(C);
		long long n_rec = 0;
		for (int pass = 0; pass < 3; ++pass) {
			const long cap = b.edge_cap;
			r = h->sx_edges.ensure(C * (size_t)cap * sizeof(StreamEdge));
			r = r ? r : h->sx_rec.ensure((size_t)b.rec_cap * sizeof(SyncState));
			r = r ? r : h->sxs_rec_src.ensure((size_t)b.rec_cap * sizeof(int));
			if (r)
				return r;
			HIP_OK(hipMemsetAsync(h->sx_counts.p, 0, 2 * C * sizeof(long long), s));
			HIP_OK(hipMemsetAsync(wb.below, 0, C * sizeof(long long), s));
			launch_bank_scan(s, h->rate, (int)C, (long)max_tiles, wb, h->sx_fn.as<StreamFn>(), h->sx_carry.as<StreamCarry>(), c_in, c_out,
				h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
			launch_bank_accept(s, h->rate, (int)C, wb, h->dev, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
			launch_bank_records(s, h->rate, (int)C, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>(), h->sxs_first.as<long long>(),
				h->sx_rec.as<SyncState>(), h->sxs_rec_src.as<int>(), dpar + P_REC_BASE * P, dpar + P_REJ_BASE * P, b.rec_cap);
			HIP_OK(hipGetLastError());
			HIP_OK(hipMemcpyAsync(counts.data(), h->sx_counts.p, 2 * C * sizeof(long long), hipMemcpyDeviceToHost, s));
			HIP_OK(hipMemcpyAsync(counts.data() + 2 * C, wb.below, C * sizeof(long long), hipMemcpyDeviceToHost, s));
			HIP_OK(hipMemcpyAsync(b.carry_h.data(), c_out, C * sizeof(StreamCarry), hipMemcpyDeviceToHost, s));
			HIP_OK(hipStreamSynchronize(s));
			b.ops += 2 + 7 + 3 + 1;
			long long most = 0;
			n_rec = 0;
			for (size_t c = 0; c < C; ++c) {
				most = std::max(most, counts[2 * c]);
				n_rec += counts[2 * c + 1];
			}
			if (most <= cap && n_rec <= b.rec_cap)
				break;
			if (pass == 2) {
				g_last_error = "bank: the edge buffers did not settle";
				return OFDMRX_E_HIP;
			}
			b.edge_cap = (long)std::max<long long>(most, cap);        // a channel with more falling edges than its share, or more records than
			b.rec_cap = (long)std::max<long long>(n_rec, b.rec_cap);  // the record buffer held: once more with room for all
		}
		for (size_t c = 0; c < C; ++c)
			if (counts[2 * C + c]) {
				g_last_error = "bank: an edge of the scan reads below the window of channel " + std::to_string(c);
				return OFDMRX_E_ARG;
			}
		std::vector<SyncState> rec((size_t)n_rec);
		if (n_rec) {
			HIP_OK(hipMemcpy(rec.data(), h->sx_rec.p, rec.size() * sizeof(SyncState), hipMemcpyDeviceToHost));
			b.ops += 1;
		}
		size_t i = 0;
		for (size_t c = 0; c < C; ++c) {
			BankChannel &k = b.ch[c];
			for (long long j = 0; j < counts[2 * c + 1]; ++j, ++i)
				k.pend.push_back(BankPending{ rec[i], -1, k.n_acc + j });
			k.n_edges += counts[2 * c];
			k.n_acc += counts[2 * c + 1];
			k.carry = b.carry_h[c];
			if (at(P_TILE_AT, c + 1) > at(P_TILE_AT, c))
				k.scanned = fin[c] ? k.fed : t_end[c] * STREAM_TILE;
		}
		b.carry_cur ^= 1;
	}
	for (size_t c = 0; c < C; ++c)
		if (fin[c] && !b.ch[c].ended)
			b.ch[c].scanned = std::max(b.ch[c].scanned, b.ch[c].fed);

	// ---- 6. one header pass over every pending preamble of a channel that goes on, whose header symbol has arrived
	std::vector<std::pair<size_t, size_t>> idx;
	for (size_t c = 0; c < C; ++c) {
		const BankChannel &k = b.ch[c];
		if (k.ended || fin[c])
			continue;
		for (size_t i = 0; i < k.pend.size(); ++i)
			if (k.pend[i].mode < 0 && k.fed >= (long long)k.pend[i].st.sc_start + L.stride + L.sl)
				idx.push_back({ c, i });
	}
	for (size_t i0 = 0; i0 < idx.size(); i0 += (size_t)h->chunk) {
		const int n = (int)std::min<size_t>((size_t)h->chunk, idx.size() - i0);
		std::vector<SyncState> st((size_t)n);
		std::vector<int> src((size_t)n);
		for (int k = 0; k < n; ++k) {
			const auto &ci = idx[i0 + (size_t)k];
			st[(size_t)k] = b.ch[ci.first].pend[ci.second].st;
			src[(size_t)k] = (int)ci.first;
			if ((r = covers(b, ci.first, (long long)st[(size_t)k].sc_start + L.stride, "the header stage")))
				return r;
		}
		r = ensure_capacity(h, n, false, 0);
		r = r ? r : b.hdr_src.ensure((size_t)h->chunk * sizeof(int));
		if (r)
			return r;
		HIP_OK(hipMemcpyAsync(h->st.p, st.data(), st.size() * sizeof(SyncState), hipMemcpyHostToDevice, s));
		HIP_OK(hipMemcpyAsync(b.hdr_src.p, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, s));
		launch_header_bank(s, h->rate, n, window_batch(b, b.hdr_src.as<int>()), h->dev, h->st.as<SyncState>(), h->hdr_soft.as<int8_t>());
		HIP_OK(hipGetLastError());
		HIP_OK(hipMemcpyAsync(st.data(), h->st.p, st.size() * sizeof(SyncState), hipMemcpyDeviceToHost, s));
		HIP_OK(hipStreamSynchronize(s));
		b.ops += 5;
		for (int k = 0; k < n; ++k) {
			const auto &ci = idx[i0 + (size_t)k];
			b.ch[ci.first].pend[ci.second].mode = st[(size_t)k].okay ? st[(size_t)k].oper_mode : 0;
		}
	}

	// ---- 7. ONE decode_records call over every record that is due on any channel, by channel, then in preamble order
	std::vector<SyncState> seeds;
	std::vector<int> seed_src;
	std::vector<int64_t> seed_index;
	for (size_t c = 0; c < C; ++c) {
		BankChannel &k = b.ch[c];
		size_t n = 0;
		for (; n < k.pend.size(); ++n) {
			const BankPending &p = k.pend[n];
			if (fin[c] || p.mode == 0)
				continue;
			// the demodulator's last symbol ends at sc_start + (rows + 2) STRIDE + SL: the last sample of the frame
			if (p.mode < 0 || k.fed < (long long)p.st.sc_start + (long long)(mode_desc(p.mode).rows + 2) * L.stride + L.sl)
				break;
		}
		if (n && (r = covers(b, c, (long long)k.pend.front().st.sc_start + L.stride, "the record pipeline")))
			return r;
		for (size_t i = 0; i < n; ++i) {
			seeds.push_back(k.pend[i].st);
			seed_src.push_back((int)c);
			seed_index.push_back(k.pend[i].index);
		}
		k.pend.erase(k.pend.begin(), k.pend.begin() + (long)n);
		if (fin[c])
			k.ended = true;
	}
	const size_t n = seeds.size();
	if (n) {
		float *const rows_user = h->esn0_user;
		r = b.seeds.ensure(n * sizeof(SyncState));
		r = r ? r : b.seed_src.ensure(n * sizeof(int));
		r = r ? r : h->sx_pay.ensure(n * PAYLOAD_BYTES);
		r = r ? r : h->sx_res.ensure(n * sizeof(Result));
		if (rows_user)
			r = r ? r : h->sx_esn0.ensure(n * ROWS_MAX * sizeof(float));
		if (r)
			return r;
		HIP_OK(hipMemcpyAsync(b.seeds.p, seeds.data(), n * sizeof(SyncState), hipMemcpyHostToDevice, s));
		HIP_OK(hipMemcpyAsync(b.seed_src.p, seed_src.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
		begin_call(h);
		r = ensure_events(h, 16);
		const WindowBatch wb = window_batch(b, nullptr);
		const RecordSources srcs{ b.seed_src.as<int>(), nullptr, 0, wb.org, wb.len };
		const FrameBatch all{ wb.samples, 0, 0, wb.fmt, 2 };          // (mono input: the analytic signal, read as I/Q pairs)
		r = r ? r : decode_records(h, all, b.seeds.as<SyncState>(), n, Outputs{ h->sx_pay.as<uint8_t>(), h->sx_res.as<Result>(), rows_user ? h->sx_esn0.as<float>() : nullptr }, srcs);
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
			BankReady q;
			q.payload.assign(pay.begin() + (long)(k * PAYLOAD_BYTES), pay.begin() + (long)((k + 1) * PAYLOAD_BYTES));
			q.res = res[k];
			if (rows_user)
				q.rows.assign(rows.begin() + (long)(k * ROWS_MAX), rows.begin() + (long)((k + 1) * ROWS_MAX));
			q.channel = seed_src[k];
			q.index = seed_index[k];
			b.ready.push_back(std::move(q));
		}
	}
	HIP_OK(hipStreamSynchronize(s));                              // (the caller's samples have left)
	b.ops += 1;
	return 0;
}

// the first max_records staged records leave; the rest wait, in order (record_channel / record_index: nullable, a feed has neither)
void deliver(ofdmrx_handle *h, size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, int32_t *record_channel, int64_t *record_index,
	size_t *n_records, size_t *n_left)
{
	ofdmrx_bank &b = *h->bank;
	size_t k = 0;
	for (; k < max_records && !b.ready.empty(); ++k) {
		const BankReady &q = b.ready.front();
		std::memcpy(payload_out + k * PAYLOAD_BYTES, q.payload.data(), PAYLOAD_BYTES);
		std::memcpy(results + k, &q.res, sizeof(Result));
		if (record_channel)
			record_channel[k] = q.channel;
		if (record_index)
			record_index[k] = q.index;
		if (h->esn0_user) {
			if (q.rows.size() == ROWS_MAX)
				std::memcpy(h->esn0_user + k * ROWS_MAX, q.rows.data(), ROWS_MAX * sizeof(float));
			else                                                      // (decoded while the rows were off)
				std::memset(h->esn0_user + k * ROWS_MAX, 0, ROWS_MAX * sizeof(float));
		}
		b.ready.pop_front();
	}
	*n_records = k;
	*n_left = b.ready.size();
}

int out_args(const ofdmrx_handle *h, size_t max_records, const void *payload, const void *results, const size_t *n_records, const size_t *n_left)
{
	if (!h || !n_records || !n_left || (max_records && (!payload || !results)))
		return OFDMRX_E_ARG;
	return 0;
}

// the handle's open bank, if it was opened as the caller's kind (a feed or a bank); else nullptr
ofdmrx_bank *live(ofdmrx_handle *h, bool as_feed)
{
	return (h && h->bank && h->bank->as_feed == as_feed) ? h->bank : nullptr;
}

int begin(ofdmrx_handle *h, size_t n_channels, int fmt, int channels, bool as_feed)
{
	if (!h || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || channels < 1 || channels > 2 || n_channels < 1 || n_channels > 65535)
		return OFDMRX_E_ARG;
	if (h->bank)                                                  // one feed or bank per handle
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	ofdmrx_bank *b = new (std::nothrow) ofdmrx_bank;
	if (!b)
		return OFDMRX_E_NOMEM;
	b->fmt = fmt;
	b->channels = channels;
	b->C = n_channels;
	b->as_feed = as_feed;
	b->ch.resize(n_channels);
	b->carry_h.assign(2 * n_channels, StreamCarry{ 0, -INFINITY, -1, 0 });
	int r = b->carry.ensure(2 * n_channels * sizeof(StreamCarry));
	if (!r && hipMemcpy(b->carry.p, b->carry_h.data(), 2 * n_channels * sizeof(StreamCarry), hipMemcpyHostToDevice) != hipSuccess)
		r = OFDMRX_E_HIP;
	if (r) {
		delete b;
		return r;
	}
	h->bank = b;
	return 0;
}

// every channel that has not ended ends: the last partial tiles, every pending preamble; what is staged leaves, and with the last
// record the bank goes
int end(ofdmrx_handle *h, ofdmrx_bank &b, size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, int32_t *record_channel,
	int64_t *record_index, size_t *n_records, size_t *n_left)
{
	HIP_OK(hipSetDevice(h->cfg.device));
	b.ops = 0;
	if (!b.ending) {
		std::vector<uint8_t> fin(b.C, 0);
		for (size_t c = 0; c < b.C; ++c)
			fin[c] = !b.ch[c].ended;
		int r = bank_step(h, nullptr, 0, nullptr, fin);
		if (r)
			return r;
		b.ending = true;
	}
	deliver(h, max_records, payload_out, results, record_channel, record_index, n_records, n_left);
	if (*n_left == 0)
		bank_free(h);
	return 0;
}

}  // namespace

extern "C" int ofdmrx_bank_begin(ofdmrx_handle *h, size_t n_channels, int fmt, int channels)
{
	return begin(h, n_channels, fmt, channels, false);
}

extern "C" int ofdmrx_bank_push(ofdmrx_handle *h, const void *samples, size_t stride_bytes, const size_t *n_samples, const uint8_t *ends,
	size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, int32_t *record_channel, int64_t *record_index, size_t *n_records,
	size_t *n_left)
{
	int r = out_args(h, max_records, payload_out, results, n_records, n_left);
	if (r || (max_records && (!record_channel || !record_index)) || !n_samples || !live(h, false) || h->bank->wide)
		return OFDMRX_E_ARG;
	ofdmrx_bank &b = *h->bank;
	const size_t unit = frame_bytes(b);
	size_t longest = 0;
	for (size_t c = 0; c < b.C; ++c) {
		if (n_samples[c] > ((size_t)1 << 26) || (n_samples[c] && (b.ch[c].ended || b.ending)))
			return OFDMRX_E_ARG;
		longest = std::max(longest, n_samples[c]);
	}
	if (longest && (!samples || (size_t)samples % unit))
		return OFDMRX_E_ARG;
	if (stride_bytes % unit || stride_bytes < longest * unit)
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	b.ops = 0;
	if (!b.ending) {
		std::vector<uint8_t> fin(b.C, 0);
		for (size_t c = 0; c < b.C && ends; ++c)
			fin[c] = ends[c] && !b.ch[c].ended;
		r = bank_step(h, (const char *)samples, stride_bytes, n_samples, fin);
		if (r)
			return r;
	}
	deliver(h, max_records, payload_out, results, record_channel, record_index, n_records, n_left);
	return 0;
}

// ---- a wideband bank: one wideband capture in, every channel made from it on the device at the reduced
// decimation p / q (q = 1: the integer decimation p); push, end and the queries serve every ratio alike
// real: the capture is real, one value per wideband position
static int begin_wideband(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int p, int q, int fmt, bool real = false)
{
	if (!h || !centre_hz || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || n_channels < 1 || n_channels > 65535)
		return OFDMRX_E_ARG;
	if (h->bank)
		return OFDMRX_E_ARG;
	if (channelize_centres(h->rate, p, q, centre_hz, n_channels, real))
		return OFDMRX_E_ARG;
	int r = begin(h, n_channels, OFDMRX_FMT_F32, 2, false);
	if (r)
		return r;
	if ((r = channelize_setup(h, p, q, centre_hz, n_channels, real))) {
		bank_free(h);
		return r;
	}
	h->bank->wide = true;
	h->bank->p = p;
	h->bank->q = q;
	h->bank->wfmt = fmt;
	h->bank->wreal = real;
	return 0;
}

extern "C" int ofdmrx_bank_begin_wideband(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int decim, int fmt)
{
	if (decim < 2 || decim > 32)
		return OFDMRX_E_ARG;
	return begin_wideband(h, n_channels, centre_hz, decim, 1, fmt);
}

extern "C" int ofdmrx_bank_begin_wideband_ratio(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int p, int q, int fmt)
{
	if (rechannelize_ratio(p, q))
		return OFDMRX_E_ARG;
	return begin_wideband(h, n_channels, centre_hz, p, q, fmt);
}

// a real capture: n_wide of ofdmrx_bank_push_wideband counts its samples, the kept tail is T - 1 of them
extern "C" int ofdmrx_bank_begin_wideband_real(ofdmrx_handle *h, size_t n_channels, const double *centre_hz, int p, int q, int fmt)
{
	if (rechannelize_ratio(p, q))
		return OFDMRX_E_ARG;
	return begin_wideband(h, n_channels, centre_hz, p, q, fmt, true);
}

// the grid front end: channel j is slot slots[j] of the raster rate / 2 (slots = NULL with n_slots = 2 decim: all)
extern "C" int ofdmrx_bank_begin_wideband_grid(ofdmrx_handle *h, size_t n_slots, const int32_t *slots, int decim, int fmt)
{
	std::vector<int32_t> list;
	if (!h || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || channelize_grid_decim(decim) || channelize_grid_slots(decim, slots, n_slots, list))
		return OFDMRX_E_ARG;
	if (h->bank)
		return OFDMRX_E_ARG;
	int r = begin(h, n_slots, OFDMRX_FMT_F32, 2, false);
	if (r)
		return r;
	if ((r = channelize_grid_setup(h, decim, list))) {
		bank_free(h);
		return r;
	}
	h->bank->wide = true;
	h->bank->p = decim;
	h->bank->q = 1;
	h->bank->wfmt = fmt;
	return 0;
}

// the same at a ratio p / q (slots = NULL with n_slots = n_all of ofdmrx_util_grid_ratio_slots: all)
extern "C" int ofdmrx_bank_begin_wideband_grid_ratio(ofdmrx_handle *h, size_t n_slots, const int32_t *slots, int p, int q, int fmt)
{
	std::vector<int32_t> list;
	if (!h || fmt < OFDMRX_FMT_S16 || fmt > OFDMRX_FMT_F32 || channelize_grid_ratio(p, q) || channelize_grid_ratio_slots(p, q, slots, n_slots, list))
		return OFDMRX_E_ARG;
	if (h->bank)
		return OFDMRX_E_ARG;
	int r = begin(h, n_slots, OFDMRX_FMT_F32, 2, false);
	if (r)
		return r;
	if ((r = channelize_grid_ratio_setup(h, p, q, list))) {
		bank_free(h);
		return r;
	}
	h->bank->wide = true;
	h->bank->p = p;
	h->bank->q = q;
	h->bank->wfmt = fmt;
	return 0;
}

extern "C" int ofdmrx_bank_push_wideband(ofdmrx_handle *h, const void *samples, size_t n_wide, int end_all, size_t max_records, uint8_t *payload_out,
	ofdmrx_frame_result *results, int32_t *record_channel, int64_t *record_index, size_t *n_records, size_t *n_left)
{
	int r = out_args(h, max_records, payload_out, results, n_records, n_left);
	if (r || (max_records && (!record_channel || !record_index)) || !live(h, false) || !h->bank->wide)
		return OFDMRX_E_ARG;
	ofdmrx_bank &b = *h->bank;
	const size_t wunit = wide_bytes(b);
	if (n_wide > ((size_t)1 << 26) || (n_wide && (!samples || (size_t)samples % wunit || b.ending || b.ch[0].ended)))
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	b.ops = 0;
	if (!b.ending) {
		// every channel takes the outputs the block completes: W samples have given ceil(W q / p) of them
		const long long P = b.p, Q = b.q;
		const std::vector<size_t> add(b.C, (size_t)(((b.wfed + (long long)n_wide) * Q + P - 1) / P - (b.wfed * Q + P - 1) / P));
		const std::vector<uint8_t> fin(b.C, (uint8_t)(end_all && !b.ch[0].ended));
		r = bank_step(h, (const char *)samples, 0, add.data(), fin, n_wide);
		if (r)
			return r;
	}
	deliver(h, max_records, payload_out, results, record_channel, record_index, n_records, n_left);
	return 0;
}

extern "C" int ofdmrx_bank_end(ofdmrx_handle *h, size_t max_records, uint8_t *payload_out, ofdmrx_frame_result *results, int32_t *record_channel,
	int64_t *record_index, size_t *n_records, size_t *n_left)
{
	int r = out_args(h, max_records, payload_out, results, n_records, n_left);
	if (r || (max_records && (!record_channel || !record_index)) || !live(h, false))
		return OFDMRX_E_ARG;
	return end(h, *h->bank, max_records, payload_out, results, record_channel, record_index, n_records, n_left);
}

extern "C" long long ofdmrx_bank_resident_samples(ofdmrx_handle *h, size_t channel)
{
	const ofdmrx_bank *b = live(h, false);
	return (b && channel < b->C) ? b->ch[channel].fed - b->ch[channel].base : OFDMRX_E_ARG;
}

extern "C" long long ofdmrx_bank_preambles(ofdmrx_handle *h, size_t channel)
{
	const ofdmrx_bank *b = live(h, false);
	return (b && channel < b->C) ? b->ch[channel].n_acc : OFDMRX_E_ARG;
}

extern "C" long long ofdmrx_bank_last_stage_ops(ofdmrx_handle *h)
{
	return live(h, false) ? h->bank->ops : OFDMRX_E_ARG;
}

// ---- ofdmrx_feed_*: one recording decoded block by block as it arrives - a bank of one channel, whose records
// come without channel and index
extern "C" int ofdmrx_feed_begin(ofdmrx_handle *h, int fmt, int channels)
{
	return begin(h, 1, fmt, channels, true);
}

extern "C" int ofdmrx_feed_push(ofdmrx_handle *h, const void *samples, size_t n_samples, size_t max_frames, uint8_t *payload_out,
	ofdmrx_frame_result *results, size_t *n_records, size_t *n_left)
{
	constexpr size_t PUSH_SLICE = (size_t)1 << 26;                // (the longest share a bank's channel takes in one step)
	int r = out_args(h, max_frames, payload_out, results, n_records, n_left);
	if (r || (n_samples && !samples) || !live(h, true))
		return OFDMRX_E_ARG;
	ofdmrx_bank &b = *h->bank;
	const size_t unit = frame_bytes(b);
	if (n_samples && (b.ending || (size_t)samples % unit))
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	b.ops = 0;
	if (!b.ending) {
		const std::vector<uint8_t> fin(1, 0);
		size_t done = 0;
		do {                                                      // (a zero-length push still takes what has become due)
			const size_t n = std::min(PUSH_SLICE, n_samples - done);
			r = bank_step(h, (const char *)samples + done * unit, 0, &n, fin);
			if (r)
				return r;
			done += n;
		} while (done < n_samples);
	}
	deliver(h, max_frames, payload_out, results, nullptr, nullptr, n_records, n_left);
	return 0;
}

extern "C" int ofdmrx_feed_end(ofdmrx_handle *h, size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_records,
	size_t *n_left)
{
	int r = out_args(h, max_frames, payload_out, results, n_records, n_left);
	if (r || !live(h, true))
		return OFDMRX_E_ARG;
	return end(h, *h->bank, max_frames, payload_out, results, nullptr, nullptr, n_records, n_left);
}

// Every kernel of the record pipeline reads inside the frame (the demodulator's last symbol ends on its last sample): no lag
extern "C" long long ofdmrx_feed_lag(ofdmrx_handle *h) { return live(h, true) ? 0 : OFDMRX_E_ARG; }

extern "C" long long ofdmrx_feed_resident_samples(ofdmrx_handle *h)
{
	return live(h, true) ? h->bank->ch[0].fed - h->bank->ch[0].base : OFDMRX_E_ARG;
}
