// api_survey.cpp -- the wideband survey behind include/ofdmrx.h: the window, ofdmrx_util_survey, and the
// band finder ofdmrx_util_find_bands (host only, float64); and the grid survey (section 4.21): ofdmrx_util_survey_grid and the slot
// finder ofdmrx_util_find_slots; and the grid survey at a ratio (section 4.24): ofdmrx_util_survey_grid_ratio and
// ofdmrx_util_find_slots_ratio.  Everything the kernels rely on is checked here, before any device call.
#include "api_internal.h"

namespace rx {

int survey_window(int nfft, float *w)
{
	const double pi = 3.14159265358979323846;
	for (int n = 0; n < nfft; ++n)
		w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)n / (double)nfft));
	return nfft;
}

static int survey_slot(int nfft) { return nfft == 1280 ? 0 : nfft == 2560 ? 1 : nfft == 5120 ? 2 : -1; }

}  // namespace rx

// the window and the roots of nfft on the device: uploaded on the first call with that length (the handle's own table belongs to
// its rate's symbol length and need not divide)
static int survey_setup(ofdmrx_handle *h, int nfft, ofdmrx_handle::SurveyPlan **out)
{
	ofdmrx_handle::SurveyPlan &p = h->survey[survey_slot(nfft)];
	*out = &p;
	if (p.u > 0.0)
		return 0;
	const double pi = 3.14159265358979323846;
	p.win_h.resize((size_t)nfft);
	survey_window(nfft, p.win_h.data());
	p.tw_h.resize((size_t)nfft);
	double u = 0.0;
	for (int n = 0; n < nfft; ++n) {
		const double a = -2.0 * pi * (double)n / (double)nfft;
		p.tw_h[(size_t)n].re = (float)std::cos(a);
		p.tw_h[(size_t)n].im = (float)std::sin(a);
		u += (double)p.win_h[(size_t)n] * (double)p.win_h[(size_t)n];
	}
	int r = p.win.ensure((size_t)nfft * sizeof(float));
	r = r ? r : p.tw.ensure((size_t)nfft * sizeof(cf));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(p.win.p, p.win_h.data(), (size_t)nfft * sizeof(float), hipMemcpyHostToDevice, h->stream));
	HIP_OK(hipMemcpyAsync(p.tw.p, p.tw_h.data(), (size_t)nfft * sizeof(cf), hipMemcpyHostToDevice, h->stream));
	p.u = u;
	return 0;
}

extern "C" int ofdmrx_util_survey_window(int nfft, float *w)
{
	if (survey_slot(nfft) < 0 || !w)
		return OFDMRX_E_ARG;
	return survey_window(nfft, w);
}

extern "C" int ofdmrx_util_survey(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int nfft,
	int segs_per_row, long long row_first, size_t n_rows, float *d_out)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (!h || !d_in || !d_out || !n_in || !n_rows || survey_slot(nfft) < 0 || segs_per_row < 1 || segs_per_row > 65536)
		return OFDMRX_E_ARG;
	if (sample_format < OFDMRX_FMT_S16 || sample_format > OFDMRX_FMT_F32 || in_first < 0 || row_first < 0)
		return OFDMRX_E_ARG;
	if (in_first > FAR || row_first > FAR || n_in > (size_t)FAR || n_rows > (size_t)FAR)
		return OFDMRX_E_ARG;
	const size_t unit = 2 * sample_bytes(sample_format);
	if ((size_t)d_in % unit || (size_t)d_out % sizeof(float))
		return OFDMRX_E_ARG;
	{
		// a position the rows need is not in the buffer: there is no zero padding
		const __int128 step = (__int128)segs_per_row * (nfft / 2);
		const __int128 lo = (__int128)row_first * step, hi = ((__int128)row_first + (__int128)n_rows) * step + nfft / 2;
		if (lo < (__int128)in_first || hi > (__int128)in_first + (__int128)n_in || hi > (__int128)FAR)
			return OFDMRX_E_ARG;
	}
	const int n_groups = (segs_per_row + SURVEY_G - 1) / SURVEY_G;
	if ((__int128)n_rows * n_groups * nfft > (__int128)survey_max_partial_floats())   // what the launch cannot hold
		return OFDMRX_E_ARG;
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		if (a < b + n_rows * (size_t)nfft * sizeof(float) && b < a + n_in * unit)
			return OFDMRX_E_ARG;
	}
	if (h->busy_live())
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	ofdmrx_handle::SurveyPlan *p = nullptr;
	int r = survey_setup(h, nfft, &p);
	r = r ? r : h->survey_part.ensure(n_rows * (size_t)n_groups * (size_t)nfft * sizeof(float));
	if (r)
		return r;
	SurveyArgs a{};
	a.in = d_in;
	a.fmt = sample_format;
	a.nfft = nfft;
	a.in_first = in_first;
	a.n_in = (long long)n_in;
	a.segs_per_row = segs_per_row;
	a.n_groups = n_groups;
	a.row_first = row_first;
	a.n_rows = (long long)n_rows;
	a.win = p->win.as<float>();
	a.tw = p->tw.as<cf>();
	a.part = h->survey_part.as<float>();
	a.out = d_out;
	launch_survey(h->stream, a, (float)(1.0 / ((double)segs_per_row * p->u)));
	HIP_OK(hipGetLastError());
	return 0;
}

extern "C" int ofdmrx_util_find_bands(const float *psd, int nfft, double rate_wide, double thr_db, double gap_hz, double min_width_hz,
	double abs_floor, size_t max_bands, ofdmrx_band *bands, size_t *n_bands, double *floor_out)
{
	if (!psd || !bands || !n_bands || survey_slot(nfft) < 0)
		return OFDMRX_E_ARG;
	if (!std::isfinite(rate_wide) || rate_wide <= 0.0 || !std::isfinite(thr_db) || thr_db < 0.0 || !std::isfinite(gap_hz) || gap_hz < 0.0)
		return OFDMRX_E_ARG;
	if (!std::isfinite(min_width_hz) || min_width_hz < 0.0 || !std::isfinite(abs_floor) || abs_floor < 0.0)
		return OFDMRX_E_ARG;
	const int N = nfft;
	std::vector<double> v(psd, psd + N);
	std::sort(v.begin(), v.end());
	const double median = 0.5 * (v[(size_t)N / 2 - 1] + v[(size_t)N / 2]);
	const double floor = std::max(median, abs_floor);
	const double level = floor * std::pow(10.0, thr_db / 10.0);
	const double bin_hz = rate_wide / (double)N;
	const double gap_bins = std::floor(gap_hz / bin_hz);          // unoccupied bins a run may bridge
	size_t count = 0;
	auto close = [&](int first, int last) {
		const double width = (double)(last - first + 1) * bin_hz;
		if (!(width >= min_width_hz))
			return;
		if (count < max_bands) {
			double sum = 0.0;
			for (int i = first; i <= last; ++i)
				sum += (double)psd[i];
			ofdmrx_band &b = bands[count];
			b.centre_hz = (0.5 * (double)(first + last) - (double)(N / 2)) * bin_hz;
			b.width_hz = width;
			b.power = sum / (double)(last - first + 1);
			b.level_db = (float)(10.0 * std::log10(b.power / floor));
			b.first_bin = first;
			b.last_bin = last;
		}
		++count;
	};
	int first = -1, last = -1;
	for (int i = 0; i < N; ++i) {
		const double p = (double)psd[i];
		if (!(p > level && p > 0.0))
			continue;
		if (first >= 0 && (double)(i - last - 1) > gap_bins) {
			close(first, last);
			first = -1;
		}
		if (first < 0)
			first = i;
		last = i;
	}
	if (first >= 0)
		close(first, last);
	*n_bands = count;
	if (floor_out)
		*floor_out = floor;
	return 0;
}

// ---- the grid survey: the mean power of every slot of the grid front end's bank, and the slot finder

extern "C" int ofdmrx_util_survey_grid(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int decim,
	int times_per_row, long long row_first, size_t n_rows, float *d_out)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (!h || !d_in || !d_out || !n_in || !n_rows || channelize_grid_decim(decim))
		return OFDMRX_E_ARG;
	if (times_per_row < SURVEY_GRID_G || times_per_row > 65536 || times_per_row % SURVEY_GRID_G)
		return OFDMRX_E_ARG;
	if (sample_format < OFDMRX_FMT_S16 || sample_format > OFDMRX_FMT_F32 || in_first < 0 || row_first < 0)
		return OFDMRX_E_ARG;
	if (in_first > FAR || row_first > FAR || n_in > (size_t)FAR || n_rows > (size_t)FAR)
		return OFDMRX_E_ARG;
	const size_t unit = 2 * sample_bytes(sample_format);
	if ((size_t)d_in % unit || (size_t)d_out % sizeof(float))
		return OFDMRX_E_ARG;
	const int M = 2 * decim;
	{
		// a position the rows need is not in the buffer: there is no zero padding other than below position 0
		const __int128 S = times_per_row, D = decim;
		__int128 lo = ((__int128)row_first * S - 24) * D;
		lo = lo < 0 ? 0 : lo;
		const __int128 hi = (((__int128)row_first + (__int128)n_rows) * S - 1) * D;
		if (lo < (__int128)in_first || hi > (__int128)in_first + (__int128)n_in - 1 || hi >= (__int128)FAR)
			return OFDMRX_E_ARG;
	}
	const int n_groups = times_per_row / SURVEY_GRID_G;
	if ((__int128)n_rows * n_groups * M > (__int128)survey_max_partial_floats())   // what the handle's partial buffer may hold
		return OFDMRX_E_ARG;
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		if (a < b + n_rows * (size_t)M * sizeof(float) && b < a + n_in * unit)
			return OFDMRX_E_ARG;
	}
	if (h->busy_live())
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	// the taps and the roots of the grid table of 4.19: the one on the device if it is a grid table of this D (whatever its slots),
	// else a new one under the usual key - a plain table of the same D is never read as a grid table, nor the reverse
	int r = 0;
	if (!(h->chz_p == decim && h->chz_q == 1 && h->chz_grid))
		r = channelize_grid_setup(h, decim, std::vector<int32_t>(1, 0));
	r = r ? r : h->survey_part.ensure(n_rows * (size_t)n_groups * (size_t)M * sizeof(float));
	if (r)
		return r;
	ChannelizeArgs t{};
	channelize_tables(h, t);
	SurveyGridArgs a{};
	a.in = d_in;
	a.fmt = sample_format;
	a.logm = grid_logm(decim);
	a.in_first = in_first;
	a.n_in = (long long)n_in;
	a.taps = t.taps;
	a.tw = t.tw;
	a.t_first = row_first * (long long)times_per_row;
	a.n_times = (long long)n_rows * (long long)times_per_row;
	a.n_groups = n_groups;
	a.n_rows = (long long)n_rows;
	a.part = h->survey_part.as<float>();
	a.out = d_out;
	launch_survey_grid(h->stream, a, (float)(1.0 / (double)times_per_row));
	HIP_OK(hipGetLastError());
	return 0;
}

extern "C" int ofdmrx_util_find_slots(const float *row, int decim, double rate, double thr_db, double sep_db, double abs_floor,
	size_t max_slots, ofdmrx_slot *slots, size_t *n_slots, double *floor_out)
{
	if (!row || !slots || !n_slots || channelize_grid_decim(decim))
		return OFDMRX_E_ARG;
	if (!std::isfinite(rate) || rate <= 0.0 || !std::isfinite(thr_db) || thr_db < 0.0 || !std::isfinite(sep_db) || sep_db < 0.0)
		return OFDMRX_E_ARG;
	if (!std::isfinite(abs_floor) || abs_floor < 0.0)
		return OFDMRX_E_ARG;
	const int M = 2 * decim;
	double floor = abs_floor;
	if (!(abs_floor > 0.0)) {
		std::vector<double> v(row, row + M);
		std::sort(v.begin(), v.end());
		floor = 0.5 * (v[(size_t)M / 2 - 1] + v[(size_t)M / 2]);
	}
	const double level = floor * std::pow(10.0, thr_db / 10.0), sep = std::pow(10.0, sep_db / 10.0);
	size_t count = 0;
	for (int i = 0; i < M; ++i) {
		const double p = (double)row[i];
		if (!(p > level && p > 0.0))
			continue;
		const double below = (double)row[(i + M - 1) % M], above = (double)row[(i + 1) % M];
		if (below > p * sep || above > p * sep)                   // shadowed: a neighbour's edge through the filter's transition band
			continue;
		if (count < max_slots) {
			ofdmrx_slot &s = slots[count];
			s.slot = i - M / 2;
			s.centre_hz = (double)(i - M / 2) * rate / 2.0;
			s.power = p;
			s.level_db = (float)(10.0 * std::log10(p / floor));
		}
		++count;
	}
	*n_slots = count;
	if (floor_out)
		*floor_out = floor;
	return 0;
}

// ---- the grid survey at a ratio: the same on the slots of the ratio grid front end's bank (4.22)

extern "C" int ofdmrx_util_survey_grid_ratio(ofdmrx_handle *h, const void *d_in, int sample_format, long long in_first, size_t n_in, int p, int q,
	int times_per_row, long long row_first, size_t n_rows, float *d_out)
{
	constexpr long long FAR = 1LL << 50;                          // positions and counts stay far inside 64 bits
	if (channelize_grid_ratio(p, q))
		return OFDMRX_E_ARG;
	if (q == 1 && !channelize_grid_decim(p))                      // 4.21 itself: its kernel, its bytes
		return ofdmrx_util_survey_grid(h, d_in, sample_format, in_first, n_in, p, times_per_row, row_first, n_rows, d_out);
	if (!h || !d_in || !d_out || !n_in || !n_rows)
		return OFDMRX_E_ARG;
	if (times_per_row < SURVEY_GRID_G || times_per_row > 65536 || times_per_row % SURVEY_GRID_G)
		return OFDMRX_E_ARG;
	if (sample_format < OFDMRX_FMT_S16 || sample_format > OFDMRX_FMT_F32 || in_first < 0 || row_first < 0)
		return OFDMRX_E_ARG;
	if (in_first > FAR || row_first > FAR || n_in > (size_t)FAR || n_rows > (size_t)FAR)
		return OFDMRX_E_ARG;
	const size_t unit = 2 * sample_bytes(sample_format);
	if ((size_t)d_in % unit || (size_t)d_out % sizeof(float))
		return OFDMRX_E_ARG;
	int32_t k_first;
	size_t n_all;
	channelize_grid_ratio_range(p, q, k_first, n_all);
	{
		// a position the rows need is not in the buffer: there is no zero padding other than below position 0
		const __int128 S = times_per_row, P = p, Q = q;
		__int128 lo = (__int128)row_first * S * P / Q - 24 * P / Q;
		lo = lo < 0 ? 0 : lo;
		const __int128 hi = (((__int128)row_first + (__int128)n_rows) * S - 1) * P / Q;
		if (lo < (__int128)in_first || hi > (__int128)in_first + (__int128)n_in - 1 || hi >= (__int128)FAR)
			return OFDMRX_E_ARG;
	}
	const int n_groups = times_per_row / SURVEY_GRID_G;
	if ((__int128)n_rows * n_groups * (__int128)n_all > (__int128)survey_max_partial_floats())   // what the handle's partial buffer may hold
		return OFDMRX_E_ARG;
	{
		const char *a = (const char *)d_in, *b = (const char *)d_out;
		if (a < b + n_rows * n_all * sizeof(float) && b < a + n_in * unit)
			return OFDMRX_E_ARG;
	}
	if (h->busy_live())
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	// the ratio-grid table of 4.22 with every slot, under the front end's key (which includes the slot list): a front-end call on other
	// slots uploads its own again, and this call after it
	std::vector<int32_t> all(n_all);
	for (size_t j = 0; j < n_all; ++j)
		all[j] = k_first + (int32_t)j;
	int r = channelize_grid_ratio_setup(h, p, q, all);
	r = r ? r : h->survey_part.ensure(n_rows * (size_t)n_groups * n_all * sizeof(float));
	if (r)
		return r;
	ChannelizeArgs t{};
	channelize_tables(h, t);
	SurveyGridRatioArgs a{};
	a.in = d_in;
	a.fmt = sample_format;
	a.p = p;
	a.q = q;
	a.in_first = in_first;
	a.n_in = (long long)n_in;
	a.taps = t.taps;
	a.tw = t.tw;
	a.inc = t.inc;
	a.n_all = (int)n_all;
	a.t_first = row_first * (long long)times_per_row;
	a.n_times = (long long)n_rows * (long long)times_per_row;
	a.n_groups = n_groups;
	a.n_rows = (long long)n_rows;
	a.part = h->survey_part.as<float>();
	a.out = d_out;
	HIP_OK(launch_survey_grid_ratio(h->stream, a, (float)(1.0 / (double)times_per_row)));
	HIP_OK(hipGetLastError());
	return 0;
}

extern "C" int ofdmrx_util_find_slots_ratio(const float *row, int p, int q, double rate, double thr_db, double sep_db, double abs_floor,
	size_t max_slots, ofdmrx_slot *slots, size_t *n_slots, double *floor_out)
{
	if (!row || !slots || !n_slots || channelize_grid_ratio(p, q))
		return OFDMRX_E_ARG;
	if (!std::isfinite(rate) || rate <= 0.0 || !std::isfinite(thr_db) || thr_db < 0.0 || !std::isfinite(sep_db) || sep_db < 0.0)
		return OFDMRX_E_ARG;
	if (!std::isfinite(abs_floor) || abs_floor < 0.0)
		return OFDMRX_E_ARG;
	int32_t k_first;
	size_t n_all;
	channelize_grid_ratio_range(p, q, k_first, n_all);
	const int N = (int)n_all;
	const bool cyclic = N * q == 2 * p;                           // the slots tile the circle: q = 1 or 2
	double floor = abs_floor;
	if (!(abs_floor > 0.0)) {
		std::vector<double> v(row, row + N);
		std::sort(v.begin(), v.end());
		floor = N & 1 ? v[(size_t)N / 2] : 0.5 * (v[(size_t)N / 2 - 1] + v[(size_t)N / 2]);
	}
	const double level = floor * std::pow(10.0, thr_db / 10.0), sep = std::pow(10.0, sep_db / 10.0);
	std::vector<char> keep((size_t)N, 0);
	for (int i = 0; i < N; ++i) {
		const double pw = (double)row[i];
		if (!(pw > level && pw > 0.0))
			continue;
		// beyond the ends of an open range lies no whole slot: a gap, or an overlap of less than a slot
		const double below = i > 0 ? (double)row[i - 1] : cyclic ? (double)row[N - 1] : 0.0;
		const double above = i < N - 1 ? (double)row[i + 1] : cyclic ? (double)row[0] : 0.0;
		if (below > pw * sep || above > pw * sep)                 // shadowed: a neighbour's edge through the filter's transition band
			continue;
		keep[(size_t)i] = 1;
	}
	// The ends seen twice.  With r = p mod q the centres of the last and the first slot lie 2 r bins apart across the band edge, a slot
	// being q bins.  Where that is half a slot or less (0 < 4 r <= q: 25/4, 9/4) each centre lies inside the other slot's own band, so a
	// signal that fits a slot reads in both at nearly the same level and two signals cannot stand there side by side: if both ends
	// passed and lie within sep_db of each other they are one signal, and the louder is reported (a tie: k_first).  Further apart than
	// sep_db they stay two, as the end rule says: neither shadows the other.
	const int r = p % q;
	if (!cyclic && r > 0 && 4 * r <= q && keep[0] && keep[(size_t)N - 1]) {
		const double a = (double)row[0], b = (double)row[N - 1];
		if (a >= b && !(a > b * sep))
			keep[(size_t)N - 1] = 0;
		else if (b > a && !(b > a * sep))
			keep[0] = 0;
	}
	size_t count = 0;
	for (int i = 0; i < N; ++i) {
		if (!keep[(size_t)i])
			continue;
		const double pw = (double)row[i];
		if (count < max_slots) {
			ofdmrx_slot &s = slots[count];
			s.slot = k_first + i;
			s.centre_hz = (double)(k_first + i) * rate / 2.0;
			s.power = pw;
			s.level_db = (float)(10.0 * std::log10(pw / floor));
		}
		++count;
	}
	*n_slots = count;
	if (floor_out)
		*floor_out = floor;
	return 0;
}
