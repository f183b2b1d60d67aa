// api_synthesize.cpp -- the wideband synthesizer behind include/ofdmrx.h (DESIGN.md sections 4.15 and 4.18): one host path for every
// interpolation p / q - ofdmrx_util_synthesize is p = interp, q = 1 of what ofdmrx_util_synthesize_ratio does, and
// launch_synthesize picks the kernel by q - and the synthesizer on a channel grid (sections 4.20 and 4.23): one call body for
// ofdmrx_util_synthesize_grid and ofdmrx_util_synthesize_grid_ratio, which picks the kernels by whether p / q is a power of two.
// Everything the kernels rely on is checked here, before any device call.
#include "api_internal.h"

// G[tn] = H[tn mod q][tn div q], tn = 0 .. 24 p, of rechannelize_taps' [q][T] -> rows b = 0 .. p - 1 of G[b + a p], a = 0 .. 24
static void resynthesize_taps(int p, int q, std::vector<float> &rows)
{
	const size_t T = (size_t)(24 * p / q + 1);
	std::vector<float> H((size_t)q * T);
	rechannelize_taps(p, q, H.data());
	rows.assign((size_t)p * RSY_ROW, 0.f);
	for (int tn = 0; tn <= 24 * p; ++tn)
		rows[(size_t)(tn % p) * RSY_ROW + (size_t)(tn / p)] = H[(size_t)(tn % q) * T + (size_t)(tn / q)];
}

// the parameters of a call on the device: the slot of the call before if nothing differs, else the next slot of the ring, once the
// last launch that read it is over (the upload reads the slot's own host copy, which nothing touches before then either)
// q = 1: the 24 p + 1 taps of the integer synthesizer at interp p; q > 1: the ratio's taps transposed, [p][RSY_ROW].  The taps lie
// behind the channels (16 bytes each), so they begin on a 16-byte boundary
// grid: a grid set (q = 1, the M / 2 = p roots of the transform behind the taps, on an 8-byte boundary); it is part
// of the key, so a grid call after a plain call at the same D uploads anew, and the reverse
// grid 2: a ratio-grid set (any q, the ratio's taps transposed, the M = 2 p roots e^{-2 pi i j / M} behind them), a
// third kind of the key: at the same (p, q) it is never taken for a grid set or a plain one
static int synthesize_setup(ofdmrx_handle *h, int p, int q, int grid, const std::vector<SynthChannel> &ch, const ofdmrx_handle::SynSlot **out)
{
	constexpr int RING = (int)(sizeof(h->syn) / sizeof(h->syn[0]));
	ofdmrx_handle::SynSlot *s = &h->syn[h->syn_cur];
	if (s->p == p && s->q == q && s->grid == grid && s->ch.size() == ch.size() && !std::memcmp(s->ch.data(), ch.data(), ch.size() * sizeof(SynthChannel))) {
		*out = s;
		return 0;
	}
	h->syn_cur = (h->syn_cur + 1) % RING;
	s = &h->syn[h->syn_cur];
	HIP_OK(hipSetDevice(h->cfg.device));
	if (s->done)
		HIP_OK(hipEventSynchronize(s->done));
	else
		HIP_OK(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
	s->p = s->q = 0;
	s->ch = ch;
	if (q == 1 && grid != 2) {
		s->taps.resize((size_t)(24 * p + 1));
		channelize_taps(p, s->taps.data());
	} else {
		resynthesize_taps(p, q, s->taps);
	}
	s->tw_at = 0;
	if (grid) {                                                   // e^{+2 pi i j / M}, j = 0 .. M / 2 - 1: the grid front end's table
		const int n_tw = grid == 2 ? 2 * p : p;                       // (grid 2: e^{-2 pi i j / M}, j = 0 .. M - 1)
		s->tw_at = (s->taps.size() + 1) / 2 * 2;
		s->taps.resize(s->tw_at + 2 * (size_t)n_tw, 0.f);
		grid_roots(p, n_tw, grid == 2, s->taps.data() + s->tw_at);
	}
	const size_t ch_bytes = ch.size() * sizeof(SynthChannel), tap_bytes = s->taps.size() * sizeof(float);
	const int r = s->dev.ensure(ch_bytes + tap_bytes);
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(s->dev.p, s->ch.data(), ch_bytes, hipMemcpyHostToDevice, h->stream));
	HIP_OK(hipMemcpyAsync((char *)s->dev.p + ch_bytes, s->taps.data(), tap_bytes, hipMemcpyHostToDevice, h->stream));
	HIP_OK(hipEventRecord(s->done, h->stream));                   // (a failed launch below still leaves the slot waitable)
	s->p = p;
	s->q = q;
	s->grid = grid;
	*out = s;
	return 0;
}

// one call at the reduced ratio p / q (q = 1: the integer interpolation p)
static int synthesize_call(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const double *centre_hz, const long long *start, const float *gain, size_t n_channels, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (!h || !d_in || !d_out || !centre_hz || !start || !gain || !n_in || !n_out || n_channels < 1 || n_channels > 65535)
		return OFDMRX_E_ARG;
	if ((in_format != OFDMRX_FMT_S16 && in_format != OFDMRX_FMT_F32) || (out_format != OFDMRX_FMT_S16 && out_format != OFDMRX_FMT_F32) ||
		in_stride < n_in || out_first < 0)
		return OFDMRX_E_ARG;
	if (out_first > FAR || in_stride > (size_t)FAR / 65536 || n_out > (size_t)synthesize_max_outputs(q))   // (n_in <= in_stride; the launch holds 2^41 - 1024 outputs)
		return OFDMRX_E_ARG;
	const size_t in_unit = 2 * sample_bytes(in_format), out_unit = 2 * sample_bytes(out_format);
	if ((size_t)d_in % in_unit || (size_t)d_out % out_unit)
		return OFDMRX_E_ARG;
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		const size_t in_bytes = ((n_channels - 1) * in_stride + n_in) * in_unit;
		if (a < b + n_out * out_unit && b < a + in_bytes)
			return OFDMRX_E_ARG;
	}
	const double d = (double)p / (double)q, rw = (double)h->rate * (double)p / (double)q;
	std::vector<SynthChannel> ch(n_channels);
	for (size_t c = 0; c < n_channels; ++c) {
		if (!std::isfinite(centre_hz[c]) || std::fabs(centre_hz[c]) > 0.5 * rw || !std::isfinite(gain[c]) || start[c] < 0 || start[c] > FAR)
			return OFDMRX_E_ARG;
		ch[c].start = start[c];
		ch[c].inc = channelize_inc(centre_hz[c], rw);
		ch[c].gain = (float)(d * (double)gain[c]);
		if (!std::isfinite(ch[c].gain))                              // (p / q x gain beyond fp32: times a zero it would not be +0)
			return OFDMRX_E_ARG;
	}
	if (h->busy_live())
		return OFDMRX_E_ARG;
	const ofdmrx_handle::SynSlot *slot = nullptr;
	int r = synthesize_setup(h, p, q, 0, ch, &slot);
	if (r)
		return r;
	HIP_OK(hipSetDevice(h->cfg.device));
	SynthesizeArgs a{};
	a.in = d_in;
	a.in_fmt = in_format;
	a.out_fmt = out_format;
	a.p = p;
	a.q = q;
	a.in_stride = (long long)in_stride;
	a.n_in = (long long)n_in;
	a.ch = slot->dev.as<SynthChannel>();
	a.taps = (const float *)((const char *)slot->dev.p + n_channels * sizeof(SynthChannel));
	a.n_channels = (int)n_channels;
	a.out_first = out_first;
	a.n_out = (long long)n_out;
	a.out = d_out;
	launch_synthesize(h->stream, a);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(slot->done, h->stream));
	return 0;
}

extern "C" int ofdmrx_util_synthesize(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int interp,
	const double *centre_hz, const long long *start, const float *gain, size_t n_channels, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	if (interp < 2 || interp > 32)
		return OFDMRX_E_ARG;
	return synthesize_call(h, d_in, in_format, in_stride, n_in, interp, 1, centre_hz, start, gain, n_channels, out_first, n_out, d_out, out_format);
}

extern "C" int ofdmrx_util_synthesize_ratio(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const double *centre_hz, const long long *start, const float *gain, size_t n_channels, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	if (rechannelize_ratio(p, q))
		return OFDMRX_E_ARG;
	return synthesize_call(h, d_in, in_format, in_stride, n_in, p, q, centre_hz, start, gain, n_channels, out_first, n_out, d_out, out_format);
}

// ---- the synthesizer on a channel grid and on a grid at a ratio (4.23): one call body.  The scratch holds V - M
// float2 per input time, two per output at an integer interpolation, 2 q at a ratio - so a call is cut into chunks of input times; a
// chunk's transform launch includes the 24 times before it, and V_j is a function of j alone, so a seam changes no byte.
// SYG_SCRATCH_BYTES bounds the scratch: well inside the 256 MiB last-level cache
#ifndef SYG_SCRATCH_BYTES
#define SYG_SCRATCH_BYTES (32u << 20)
#endif

// q = 1 with p a power of two is 4.20 itself: its set, its kernels, its bytes
static bool is_plain_grid(int p, int q) { return q == 1 && !channelize_grid_decim(p); }

// output times per chunk at interpolation D: whole tiles of the filter kernel, with the 24 times of history and the round-up to
// whole tiles of the transform kernel inside the bound
static long long synthesize_grid_chunk_times(int D)
{
	const long long per_time = 2LL * D * (long long)sizeof(float2), tile = synthesize_grid_tile_times(D), ft = synthesize_grid_filter_times(D);
	const long long fit = ((long long)SYG_SCRATCH_BYTES / per_time - 24 - tile) / ft * ft;
	return fit > ft ? fit : ft;
}

// input times per chunk at the ratio p / q: a multiple of q - so a chunk is a whole number of outputs, times / q x p - with the 24
// times of history and the round-up to whole tiles of the transform kernel inside the bound
static long long synthesize_grid_ratio_chunk_times(int p, int q)
{
	const long long per_time = 2LL * p * (long long)sizeof(float2), tile = synthesize_grid_ratio_tile_times(p, q);
	const long long round = synthesize_grid_ratio_filter_round(q);  // (q = 1: the filter's work items take 8 output times each)
	const long long fit = ((long long)SYG_SCRATCH_BYTES / per_time - 24 - tile - (round - 1)) / q * q;
	return fit > q ? fit : q;
}

extern "C" long long ofdmrx_util_synthesize_grid_chunk(int interp)
{
	if (channelize_grid_decim(interp))
		return OFDMRX_E_ARG;
	return synthesize_grid_chunk_times(interp) * interp;
}

extern "C" long long ofdmrx_util_synthesize_grid_ratio_chunk(int p, int q)
{
	if (channelize_grid_ratio(p, q))
		return OFDMRX_E_ARG;
	if (is_plain_grid(p, q))
		return synthesize_grid_chunk_times(p) * p;
	return synthesize_grid_ratio_chunk_times(p, q) / q * p;
}

// the chunks of a plain grid call (4.20): ranges of output times
static int synthesize_grid_launches(ofdmrx_handle *h, const ofdmrx_handle::SynSlot *slot, SynthesizeGridArgs a)
{
	const int D = a.p, M = 2 * D;
	const long long q_lo = a.out_first / D, q_hi = (a.out_first + a.n_out - 1) / D, nq_all = q_hi - q_lo + 1;
	const long long chunk = synthesize_grid_chunk_times(D), tile = synthesize_grid_tile_times(D);
	// the times a launch's scratch holds: the chunk's own, rounded up to the filter's 8 per work item, the 24 before, whole tiles
	auto times_of = [&](long long nq) { return ((nq + 7) / 8 * 8 + 24 + tile - 1) / tile * tile; };
	const int r = h->syn_scratch.ensure((size_t)times_of(nq_all < chunk ? nq_all : chunk) * (size_t)M * sizeof(float2));
	if (r)
		return r;
	a.tw = (const float2 *)(a.taps + slot->tw_at);
	a.scratch = h->syn_scratch.as<float2>();
	for (long long at = 0; at < nq_all; at += chunk) {
		const long long nq = nq_all - at < chunk ? nq_all - at : chunk;
		a.q_first = q_lo + at;
		a.j_first = a.q_first - 24;
		a.nq = (int)nq;
		a.n_times = (int)times_of(nq);
		launch_synthesize_grid(h->stream, a);
		HIP_OK(hipGetLastError());
	}
	return 0;
}

// the chunks of a ratio-grid call (4.23): ranges of input times J = (m q) div p, counted from out_first rounded down to a multiple
// of p; chunk i holds the outputs base + i C .. base + (i + 1) C - 1, C = ofdmrx_util_synthesize_grid_ratio_chunk(p, q)
static int synthesize_grid_ratio_launches(ofdmrx_handle *h, const ofdmrx_handle::SynSlot *slot, SynthesizeGridRatioArgs a)
{
	const int p = a.p, q = a.q, M = 2 * p;
	const long long chunk_j = synthesize_grid_ratio_chunk_times(p, q), chunk_m = chunk_j / q * p, tile = synthesize_grid_ratio_tile_times(p, q);
	const long long base = a.out_first / p * p, hi = a.out_first + a.n_out;
	const long long round = synthesize_grid_ratio_filter_round(q);
	// the times a launch's scratch holds: the 24 before the first output's, the outputs' own - rounded up to what a work item of
	// the filter takes - whole tiles
	auto times_of = [&](long long m_first, long long n_m) {
		const long long j_lo = m_first * q / p, j_hi = (m_first + n_m - 1) * q / p;
		return ((j_hi - j_lo + round) / round * round + 24 + tile - 1) / tile * tile;
	};
	// (a chunk's own range of times lies inside its whole chunk's, and every whole chunk has the same number)
	const long long most = hi - base <= chunk_m ? times_of(a.out_first, a.n_out) : times_of(base, chunk_m);
	const int r = h->syn_scratch.ensure((size_t)most * (size_t)M * sizeof(float2));
	if (r)
		return r;
	a.tw = (const float2 *)(a.taps + slot->tw_at);
	a.scratch = h->syn_scratch.as<float2>();
	for (long long at = base; at < hi; at += chunk_m) {
		const long long lo = at > a.out_first ? at : a.out_first, end = at + chunk_m < hi ? at + chunk_m : hi;
		a.m_first = lo;
		a.n_m = end - lo;
		a.j_first = lo * q / p - 24;
		a.n_times = (int)times_of(lo, a.n_m);
		launch_synthesize_grid_ratio(h->stream, a);
		HIP_OK(hipGetLastError());
	}
	return 0;
}

// one call at the reduced ratio p / q, which the caller has checked (channelize_grid_decim(p) with q = 1, or channelize_grid_ratio)
static int synthesize_grid_call(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const int32_t *slots, const long long *start, const float *gain, size_t n_slots, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (!h || !d_in || !d_out || !start || !gain || !n_in || !n_out)
		return OFDMRX_E_ARG;
	const bool plain = is_plain_grid(p, q);
	const int M = 2 * p;
	int32_t k_first;
	size_t n_all;
	channelize_grid_ratio_range(p, q, k_first, n_all);            // (q = 1: -p .. p - 1, all M of them)
	if (n_slots < 1 || n_slots > n_all || (!slots && n_slots != n_all))
		return OFDMRX_E_ARG;
	if ((in_format != OFDMRX_FMT_S16 && in_format != OFDMRX_FMT_F32) || (out_format != OFDMRX_FMT_S16 && out_format != OFDMRX_FMT_F32) ||
		in_stride < n_in || out_first < 0)
		return OFDMRX_E_ARG;
	// n_out: the filter's launch holds 2^31 - 1 tiles of 1024 outputs a chunk, and a chunk is far smaller; (out_first + n_out) q stays
	// below 2^55.  The bound is the other synthesizers': 1024 (2^31 - 1)
	if (out_first > FAR || in_stride > (size_t)FAR / 65536 || n_out > (size_t)synthesize_max_outputs(1))
		return OFDMRX_E_ARG;
	const size_t in_unit = 2 * sample_bytes(in_format), out_unit = 2 * sample_bytes(out_format);
	if ((size_t)d_in % in_unit || (size_t)d_out % out_unit)
		return OFDMRX_E_ARG;
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		const size_t in_bytes = ((n_slots - 1) * in_stride + n_in) * in_unit;
		if (a < b + n_out * out_unit && b < a + in_bytes)
			return OFDMRX_E_ARG;
	}
	std::vector<int32_t> slot_list;
	if (channelize_grid_ratio_slots(p, q, slots, n_slots, slot_list))
		return OFDMRX_E_ARG;
	const unsigned step = (unsigned)(4294967296ULL / (unsigned long long)M);
	const GridRatioPlan pl = plain ? GridRatioPlan{} : channelize_grid_ratio_plan(p, q);
	const double d = (double)p / (double)q;
	std::vector<SynthChannel> ch(n_slots);
	std::vector<char> taken(n_all, 0);
	for (size_t c = 0; c < n_slots; ++c) {
		char &t = taken[(size_t)(slot_list[c] - k_first)];
		if (t || !std::isfinite(gain[c]) || start[c] < 0 || start[c] > FAR || start[c] % p)
			return OFDMRX_E_ARG;                                      // a slot given twice; a start that p does not divide
		t = 1;
		if (plain) {
			ch[c].start = start[c];
			ch[c].inc = (unsigned)slot_list[c] * step;                // k 2^32 / M mod 2^32: what channelize_inc gives for k rate / 2, without a rounding
		} else {
			const int k = slot_list[c], bin = ((-k) % M + M) % M;
			ch[c].start = start[c] / p * q;                           // the row's first input time
			ch[c].inc = (unsigned)channelize_grid_ratio_row(pl, bin) | (unsigned)(k & 1) << 16;
		}
		ch[c].gain = (float)(d * (double)gain[c]);
		if (!std::isfinite(ch[c].gain))
			return OFDMRX_E_ARG;
	}
	if (h->busy_live())
		return OFDMRX_E_ARG;
	const ofdmrx_handle::SynSlot *slot = nullptr;
	int r = synthesize_setup(h, p, q, plain ? 1 : 2, ch, &slot);
	if (r)
		return r;
	HIP_OK(hipSetDevice(h->cfg.device));
	const SynthChannel *d_ch = slot->dev.as<SynthChannel>();
	const float *d_taps = (const float *)((const char *)slot->dev.p + n_slots * sizeof(SynthChannel));
	if (plain) {
		SynthesizeGridArgs a{};
		a.in = d_in;
		a.in_fmt = in_format;
		a.out_fmt = out_format;
		a.p = p;
		a.in_stride = (long long)in_stride;
		a.n_in = (long long)n_in;
		a.ch = d_ch;
		a.taps = d_taps;
		a.n_channels = (int)n_slots;
		a.out_first = out_first;
		a.n_out = (long long)n_out;
		a.out = d_out;
		r = synthesize_grid_launches(h, slot, a);
	} else {
		SynthesizeGridRatioArgs a{};
		a.in = d_in;
		a.in_fmt = in_format;
		a.out_fmt = out_format;
		a.p = p;
		a.q = q;
		a.in_stride = (long long)in_stride;
		a.n_in = (long long)n_in;
		a.ch = d_ch;
		a.taps = d_taps;
		a.n_channels = (int)n_slots;
		a.out_first = out_first;
		a.n_out = (long long)n_out;
		a.out = d_out;
		r = synthesize_grid_ratio_launches(h, slot, a);
	}
	if (r)
		return r;
	HIP_OK(hipEventRecord(slot->done, h->stream));
	return 0;
}

extern "C" int ofdmrx_util_synthesize_grid(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int interp,
	const int32_t *slots, const long long *start, const float *gain, size_t n_slots, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	if (channelize_grid_decim(interp))
		return OFDMRX_E_ARG;
	return synthesize_grid_call(h, d_in, in_format, in_stride, n_in, interp, 1, slots, start, gain, n_slots, out_first, n_out, d_out, out_format);
}

extern "C" int ofdmrx_util_synthesize_grid_ratio(ofdmrx_handle *h, const void *d_in, int in_format, size_t in_stride, size_t n_in, int p, int q,
	const int32_t *slots, const long long *start, const float *gain, size_t n_slots, long long out_first, size_t n_out, void *d_out,
	int out_format)
{
	if (channelize_grid_ratio(p, q))
		return OFDMRX_E_ARG;
	return synthesize_grid_call(h, d_in, in_format, in_stride, n_in, p, q, slots, start, gain, n_slots, out_first, n_out, d_out, out_format);
}
