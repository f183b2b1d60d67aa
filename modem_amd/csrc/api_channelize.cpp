// api_channelize.cpp -- the wideband front end behind include/ofdmrx.h (DESIGN.md sections 4.14 and 4.17): the taps, the phase
// increments, and one host path for every decimation p / q - ofdmrx_util_channelize is p = decim, q = 1 of what
// ofdmrx_util_channelize_ratio does, and launch_channelize picks the kernel by q.  ofdmrx_util_channelize_real (section 4.25) is the
// same path with a flag, down to launch_channelize: a real capture, one value per position, the same taps and increments, its own
// rule for the centres.
// Everything the kernels rely on is checked here, before any device call.
#include "api_internal.h"

namespace rx {

int channelize_taps(int decim, float *taps)
{
	const int D = decim, K = 12 * D, T = 2 * K + 1;
	const double pi = 3.14159265358979323846;
	std::vector<double> h((size_t)T);
	double sum = 0.0;
	for (int k = 0; k < T; ++k) {
		const double t = 0.75 * (double)(k - K) / (double)D;
		const double sinc = k == K ? 1.0 : std::sin(pi * t) / (pi * t);
		const double w = 0.42 - 0.5 * std::cos(2.0 * pi * (double)k / (double)(T - 1)) + 0.08 * std::cos(4.0 * pi * (double)k / (double)(T - 1));
		h[(size_t)k] = 0.75 / (double)D * sinc * w;
		sum += h[(size_t)k];
	}
	for (int k = 0; k < T; ++k)
		taps[k] = (float)(h[(size_t)k] / sum);
	return T;
}

unsigned channelize_inc(double centre_hz, double rw)
{
	return (unsigned)(unsigned long long)std::llrint(centre_hz * 4294967296.0 / rw);
}

// the same at a rational decimation p / q, one row of T = 24 p div q + 1 taps per phase r = 0 .. q - 1:
// h_r[j] = g(j + r / q - K), K = 12 p / q, g(t) = sinc(0.75 t / D) (0.42 + 0.5 cos(pi t / K) + 0.08 cos(2 pi t / K)) inside |t| <= K:
// with the integer tn = j q + r - 12 p the time is t = tn / q, t / D = tn / p and t / K = tn / (12 p)
int rechannelize_taps(int p, int q, float *taps)
{
	if (q == 1)
		return channelize_taps(p, taps);
	const int T = 24 * p / q + 1;
	const double pi = 3.14159265358979323846;
	std::vector<double> h((size_t)T);
	for (int r = 0; r < q; ++r) {
		double sum = 0.0;
		for (int j = 0; j < T; ++j) {
			const long tn = (long)j * q + r - 12L * p;
			double v = 0.0;
			if (std::labs(tn) <= 12L * p) {
				const double x = 0.75 * (double)tn / (double)p, y = (double)tn / (double)(12L * p);
				const double sinc = tn == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
				v = sinc * (0.42 + 0.5 * std::cos(pi * y) + 0.08 * std::cos(2.0 * pi * y));
			}
			h[(size_t)j] = v;
			sum += v;
		}
		for (int j = 0; j < T; ++j)
			taps[(size_t)r * (size_t)T + (size_t)j] = (float)(h[(size_t)j] / sum);
	}
	return T;
}

}  // namespace rx

int reduce_ratio(int &p, int &q)
{
	if (p <= 0 || q <= 0)
		return OFDMRX_E_ARG;
	int a = p, b = q;
	while (b) {
		const int t = a % b;
		a = b;
		b = t;
	}
	p /= a;
	q /= a;
	return 0;
}

int rechannelize_ratio(int &p, int &q)
{
	if (reduce_ratio(p, q) || q > 16 || p < 2 * q || p > 32 * q)
		return OFDMRX_E_ARG;
	return 0;
}

void grid_roots(int p, int n, bool negative, float *dst)
{
	const double pi = 3.14159265358979323846;
	for (int j = 0; j < n; ++j) {
		const double s = std::sin(pi * (double)j / (double)p);
		dst[2 * j] = (float)std::cos(pi * (double)j / (double)p);
		dst[2 * j + 1] = (float)(negative ? -s : s);
	}
}

// the taps of the reduced ratio p / q and the increments of the centres on the device.  What is there already stays (a bank's pushes,
// a capture cut into blocks); anything else - other centres, another ratio, an integer decimation after a ratio - waits for the
// stream first, since a kernel enqueued earlier may still read the old values.  The device holds the taps transposed, [T][q], as
// k_rechannelize reads them; at q = 1 that is channelize_taps' own order, which k_channelize reads
// grid: a grid table (q = 1, the M / 2 = p roots of the transform behind the taps); it is part of the key, so a
// grid call after a plain call at the same D uploads again, and the reverse
// grid 2: a ratio-grid table (any q, the M = 2 p roots e^{-2 pi i j / M} behind the taps), a third kind of the key
static int channelize_upload(ofdmrx_handle *h, int p, int q, int grid, const std::vector<unsigned> &inc)
{
	if (p == h->chz_p && q == h->chz_q && grid == h->chz_grid && inc == h->chz_inc_h)
		return 0;
	HIP_OK(hipSetDevice(h->cfg.device));
	HIP_OK(hipStreamSynchronize(h->stream));
	h->chz_p = h->chz_q = 0;
	const size_t T = (size_t)(24 * p / q + 1);
	std::vector<float> rows((size_t)q * T);
	rechannelize_taps(p, q, rows.data());
	h->chz_taps_h.resize(rows.size());
	for (size_t r = 0; r < (size_t)q; ++r)
		for (size_t j = 0; j < T; ++j)
			h->chz_taps_h[j * (size_t)q + r] = rows[r * T + j];
	h->chz_tw_at = 0;
	if (grid) {                                                   // e^{+2 pi i j / M}, j = 0 .. M / 2 - 1, on an 8-byte boundary
		const int n_tw = grid == 2 ? 2 * p : p;                       // (grid 2: e^{-2 pi i j / M}, j = 0 .. M - 1)
		h->chz_tw_at = ((size_t)q * T + 1) / 2 * 2;
		h->chz_taps_h.resize(h->chz_tw_at + 2 * (size_t)n_tw, 0.f);
		grid_roots(p, n_tw, grid == 2, h->chz_taps_h.data() + h->chz_tw_at);
	}
	h->chz_inc_h = inc;
	int r = h->chz_taps.ensure(h->chz_taps_h.size() * sizeof(float));
	r = r ? r : h->chz_inc.ensure(inc.size() * sizeof(unsigned));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(h->chz_taps.p, h->chz_taps_h.data(), h->chz_taps_h.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
	HIP_OK(hipMemcpyAsync(h->chz_inc.p, h->chz_inc_h.data(), inc.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
	h->chz_p = p;
	h->chz_q = q;
	h->chz_grid = grid;
	return 0;
}

// the centres a front end at p / q takes: finite and inside +- Rw / 2.  real: a real capture holds every signal at
// +f and its conjugate at -f, and the pass band is flat to rate / 4 on either side of a centre, so a centre with |f| < rate / 4 (the
// mirror across 0) or |f| > Rw / 2 - rate / 4 (the mirror across Rw / 2) has the mirror's pass band over its own: refused
int channelize_centres(int rate, int p, int q, const double *centre_hz, size_t n_channels, bool real)
{
	const double rw = (double)rate * (double)p / (double)q, edge = 0.25 * (double)rate;
	for (size_t c = 0; c < n_channels; ++c) {
		const double f = std::fabs(centre_hz[c]);
		if (!std::isfinite(f) || f > 0.5 * rw || (real && (f < edge || f > 0.5 * rw - edge)))
			return OFDMRX_E_ARG;
	}
	return 0;
}

// (a real capture's taps and increments are the analytic ones: the device tables do not know the kind of the capture)
int channelize_setup(ofdmrx_handle *h, int p, int q, const double *centre_hz, size_t n_channels, bool real)
{
	if (channelize_centres(h->rate, p, q, centre_hz, n_channels, real))
		return OFDMRX_E_ARG;
	const double rw = (double)h->rate * (double)p / (double)q;
	std::vector<unsigned> inc(n_channels);
	for (size_t c = 0; c < n_channels; ++c)
		inc[c] = channelize_inc(centre_hz[c], rw);
	return channelize_upload(h, p, q, 0, inc);
}

int channelize_grid_decim(int decim)
{
	return (decim >= 2 && decim <= 512 && !(decim & (decim - 1))) ? 0 : OFDMRX_E_ARG;
}

int channelize_grid_slots(int decim, const int32_t *slots, size_t n_slots, std::vector<int32_t> &out)
{
	const int M = 2 * decim;
	if (n_slots < 1 || n_slots > 65535 || (!slots && n_slots != (size_t)M))
		return OFDMRX_E_ARG;
	out.resize(n_slots);
	for (size_t j = 0; j < n_slots; ++j) {
		out[j] = slots ? slots[j] : (int32_t)j - M / 2;
		if (out[j] < -M / 2 || out[j] > M / 2 - 1)
			return OFDMRX_E_ARG;
	}
	return 0;
}

// slot k's increment k 2^32 / M mod 2^32: what channelize_inc gives for the centre k rate / 2, without a rounding
int channelize_grid_setup(ofdmrx_handle *h, int decim, const std::vector<int32_t> &slots)
{
	const unsigned step = (unsigned)(4294967296ULL / (unsigned long long)(2 * decim));
	std::vector<unsigned> inc(slots.size());
	for (size_t j = 0; j < slots.size(); ++j)
		inc[j] = (unsigned)slots[j] * step;
	return channelize_upload(h, decim, 1, 1, inc);
}

// the grid front end at a ratio: p / q reduced here; 1 <= q <= 16, 2 q <= p <= 512, p = 2^a 3^b 5^c
int channelize_grid_ratio(int &p, int &q)
{
	if (reduce_ratio(p, q) || q > 16 || p < 2 * q || p > 512)
		return OFDMRX_E_ARG;
	int m = p;
	for (int f : { 2, 3, 5 })
		while (m % f == 0)
			m /= f;
	return m == 1 ? 0 : OFDMRX_E_ARG;
}

// its slots: the k with -p <= k q < p, k_first = -(p div q) .. ceil(p / q) - 1
void channelize_grid_ratio_range(int p, int q, int32_t &k_first, size_t &n_all)
{
	k_first = -(p / q);
	n_all = (size_t)((p + q - 1) / q + p / q);
}

int channelize_grid_ratio_slots(int p, int q, const int32_t *slots, size_t n_slots, std::vector<int32_t> &out)
{
	int32_t k_first;
	size_t n_all;
	channelize_grid_ratio_range(p, q, k_first, n_all);
	if (n_slots < 1 || n_slots > 65535 || (!slots && n_slots != n_all))
		return OFDMRX_E_ARG;
	out.resize(n_slots);
	for (size_t j = 0; j < n_slots; ++j) {
		out[j] = slots ? slots[j] : k_first + (int32_t)j;
		if (out[j] < k_first || out[j] > k_first + (int32_t)n_all - 1)
			return OFDMRX_E_ARG;
	}
	return 0;
}

// q = 1 with p a power of two is 4.19 itself: its table, its kernel, its bytes
static bool is_plain_grid(int p, int q) { return q == 1 && !channelize_grid_decim(p); }

int channelize_grid_ratio_setup(ofdmrx_handle *h, int p, int q, const std::vector<int32_t> &slots)
{
	if (is_plain_grid(p, q))
		return channelize_grid_setup(h, p, slots);
	const GridRatioPlan pl = channelize_grid_ratio_plan(p, q);
	std::vector<unsigned> inc(slots.size());
	for (size_t j = 0; j < slots.size(); ++j) {
		const int kq = ((slots[j] * q) % pl.m + pl.m) % pl.m;
		inc[j] = (unsigned)channelize_grid_ratio_row(pl, (pl.m - kq) % pl.m) | (unsigned)kq << 16;
	}
	return channelize_upload(h, p, q, 2, inc);
}

void launch_channelize_any(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.grid == 2)
		launch_channelize_grid_ratio(s, a);
	else if (a.grid)
		launch_channelize_grid(s, a);
	else
		launch_channelize(s, a);
}

void channelize_tables(const ofdmrx_handle *h, ChannelizeArgs &a)
{
	a.taps = h->chz_taps.as<float>();
	a.inc = h->chz_inc.as<unsigned>();
	a.grid = h->chz_grid;
	a.tw = h->chz_grid ? (const float2 *)(h->chz_taps.as<float>() + h->chz_tw_at) : nullptr;
}

extern "C" int ofdmrx_util_channelize_taps(int decim, float *taps)
{
	if (decim < 2 || decim > 32 || !taps)
		return OFDMRX_E_ARG;
	return channelize_taps(decim, taps);
}

extern "C" int ofdmrx_util_channelize_ratio_taps(int p, int q, float *taps)
{
	if (rechannelize_ratio(p, q) || !taps)
		return OFDMRX_E_ARG;
	return rechannelize_taps(p, q, taps);
}

// one call at the reduced ratio p / q (q = 1: the integer decimation p).  grid: the grid front end at decimation p / q, whose channels
// are the slots (nullable: all of them) and not centres - section 4.19's where q = 1 and p is a power of two, else section 4.22's
// real: d_in is a real capture, one value per wideband position (section 4.25; not with grid)
static int channelize_call(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride,
	bool grid = false, const int32_t *slots = nullptr, bool real = false)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (!h || !d_in || !d_out || (!grid && !centre_hz) || !n_in || !n_out || n_channels < 1 || n_channels > 65535)
		return OFDMRX_E_ARG;
	if (sample_format < OFDMRX_FMT_S16 || sample_format > OFDMRX_FMT_F32 || in_first < 0 || out_first < 0 || out_stride < n_out)
		return OFDMRX_E_ARG;
	if (in_first > FAR || out_first > FAR || n_in > (size_t)FAR || n_out > (size_t)(!grid ? channelize_max_outputs(q) : is_plain_grid(p, q) ? channelize_grid_max_outputs() : channelize_grid_ratio_max_outputs()) || out_stride > (size_t)FAR / 65536)
		return OFDMRX_E_ARG;
	const size_t unit = (real ? 1 : 2) * sample_bytes(sample_format);
	if ((size_t)d_in % unit || (size_t)d_out % sizeof(float2))
		return OFDMRX_E_ARG;
	const long long P = p, Q = q, T = 24 * P / Q + 1;
	if ((in_first > 0 && out_first * P / Q - (T - 1) < in_first) || (out_first + (long long)n_out - 1) * P / Q > in_first + (long long)n_in - 1)
		return OFDMRX_E_ARG;                                      // a position the outputs need is not in the buffer
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		const size_t out_bytes = ((n_channels - 1) * out_stride + n_out) * sizeof(float2);
		if (a < b + out_bytes && b < a + n_in * unit)
			return OFDMRX_E_ARG;
	}
	std::vector<int32_t> slot_list;
	if (grid && channelize_grid_ratio_slots(p, q, slots, n_channels, slot_list))
		return OFDMRX_E_ARG;
	for (size_t c = 0; c < n_channels && !grid; ++c)
		if (!std::isfinite(centre_hz[c]))
			return OFDMRX_E_ARG;
	if (real && channelize_centres(h->rate, p, q, centre_hz, n_channels, true))
		return OFDMRX_E_ARG;
	if (h->busy_live())                                           // (an open wideband bank owns the taps and increments on the device)
		return OFDMRX_E_ARG;
	int r = grid ? channelize_grid_ratio_setup(h, p, q, slot_list) : channelize_setup(h, p, q, centre_hz, n_channels, real);
	if (r)
		return r;
	HIP_OK(hipSetDevice(h->cfg.device));
	ChannelizeArgs a{};
	a.in = d_in;
	a.fmt = sample_format;
	a.p = p;
	a.q = q;
	a.in_first = in_first;
	a.n_in = (long long)n_in;
	channelize_tables(h, a);
	a.n_channels = (int)n_channels;
	a.out_first = out_first;
	a.n_out = (long long)n_out;
	a.out = d_out;
	a.out_stride = (long long)out_stride;
	a.dst = nullptr;
	a.real = real;
	launch_channelize_any(h->stream, a);
	HIP_OK(hipGetLastError());
	return 0;
}

extern "C" int ofdmrx_util_channelize(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride)
{
	if (decim < 2 || decim > 32)
		return OFDMRX_E_ARG;
	return channelize_call(h, d_in, sample_format, in_first, n_in, decim, 1, centre_hz, n_channels, out_first, n_out, d_out, out_stride);
}

extern "C" int ofdmrx_util_channelize_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride)
{
	if (rechannelize_ratio(p, q))
		return OFDMRX_E_ARG;
	return channelize_call(h, d_in, sample_format, in_first, n_in, p, q, centre_hz, n_channels, out_first, n_out, d_out, out_stride);
}

// the front end for a real capture: one entry for every ratio, q = 1 the integer decimation
extern "C" int ofdmrx_util_channelize_real(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const double *centre_hz, size_t n_channels, long long out_first, size_t n_out, float *d_out, size_t out_stride)
{
	if (rechannelize_ratio(p, q))
		return OFDMRX_E_ARG;
	return channelize_call(h, d_in, sample_format, in_first, n_in, p, q, centre_hz, n_channels, out_first, n_out, d_out, out_stride, false, nullptr, true);
}

extern "C" int ofdmrx_util_channelize_grid_taps(int decim, float *taps)
{
	if (channelize_grid_decim(decim) || !taps)
		return OFDMRX_E_ARG;
	return channelize_taps(decim, taps);
}

extern "C" int ofdmrx_util_channelize_grid(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	const int32_t *slots, size_t n_slots, long long out_first, size_t n_out, float *d_out, size_t out_stride)
{
	if (channelize_grid_decim(decim))
		return OFDMRX_E_ARG;
	return channelize_call(h, d_in, sample_format, in_first, n_in, decim, 1, nullptr, n_slots, out_first, n_out, d_out, out_stride, true, slots);
}

// the grid front end at a ratio
extern "C" int ofdmrx_util_channelize_grid_ratio_taps(int p, int q, float *taps)
{
	if (channelize_grid_ratio(p, q) || !taps)
		return OFDMRX_E_ARG;
	return rechannelize_taps(p, q, taps);
}

extern "C" int ofdmrx_util_grid_ratio_slots(int p, int q, int32_t *k_first, size_t *n_all)
{
	if (channelize_grid_ratio(p, q) || !k_first || !n_all)
		return OFDMRX_E_ARG;
	channelize_grid_ratio_range(p, q, *k_first, *n_all);
	return 0;
}

extern "C" int ofdmrx_util_channelize_grid_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	const int32_t *slots, size_t n_slots, long long out_first, size_t n_out, float *d_out, size_t out_stride)
{
	if (channelize_grid_ratio(p, q))
		return OFDMRX_E_ARG;
	return channelize_call(h, d_in, sample_format, in_first, n_in, p, q, nullptr, n_slots, out_first, n_out, d_out, out_stride, true, slots);
}
