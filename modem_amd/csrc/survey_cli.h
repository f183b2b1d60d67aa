// survey_cli.h -- what `survey` and `decode_stream --wideband DECIM|P/Q auto` share: the decimation argument, and the occupied bands
// of a whole wideband capture
// (ofdmrx_util_survey + ofdmrx_util_find_bands) with the finder's default parameters; and what `survey --grid`
// and `decode_stream --grid DECIM auto[:FLOOR_DB]` share: the occupied slots of a whole grid capture (section 4.21); and the same at a
// ratio for `survey --grid-ratio` and `decode_stream --grid-ratio P/Q auto[:FLOOR_DB]` (section 4.24).
#pragma once
#include "wav_read.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

constexpr double SURVEY_THR_DB = 6.0, SURVEY_GAP_HZ = 200.0, SURVEY_MIN_WIDTH_HZ = 1000.0;

// The decimation argument of both programs: DECIM, an integer 2 .. 32, or - when it holds a '/' - a ratio P/Q (DESIGN.md section
// 4.17: lowest terms Q <= 16, 2 <= P / Q <= 32).  valid(): in range.  rate_of(): the handle rate wide_rate Q / P, 0 if that is no integer.
struct Decimation {
	int p = 0, q = 1;
	bool ratio = false;
	explicit Decimation(const char *arg)
	{
		const char *slash = std::strchr(arg, '/');
		p = std::atoi(arg);
		ratio = slash != nullptr;
		if (ratio)
			q = std::atoi(slash + 1);
	}
	bool valid() const
	{
		if (!ratio)
			return p >= 2 && p <= 32;
		if (p <= 0 || q <= 0)
			return false;
		int a = p, b = q;
		while (b) {
			const int t = a % b;
			a = b;
			b = t;
		}
		return q / a <= 16 && p >= 2 * q && p <= 32 * q;
	}
	int rate_of(int wide_rate) const
	{
		const long long num = (long long)wide_rate * q;
		return (p > 0 && num % p == 0) ? (int)(num / p) : 0;
	}
};

// w: a 2-channel capture read by read_wav.  One spectrum over the whole file: rows of at most 65536 segments, averaged here in double
// when there are several.  Returns false with a message on stderr; bands may come back empty.
static bool survey_capture(ofdmrx_handle *h, const Wav &w, int nfft, std::vector<ofdmrx_band> &bands, double &floor)
{
	const size_t hop = (size_t)nfft / 2;
	const size_t total = w.frames >= (size_t)nfft ? (w.frames - hop) / hop : 0;
	if (!total) {
		std::fprintf(stderr, "The capture is shorter than one segment of %d samples.\n", nfft);
		return false;
	}
	const size_t S = std::min<size_t>(total, 65536), n_rows = total / S;
	const size_t in_bytes = w.pcm.size();
	void *d_in = nullptr, *d_out = nullptr;
	std::vector<float> rows(n_rows * (size_t)nfft);
	hipError_t e = hipMalloc(&d_in, in_bytes);
	e = e == hipSuccess ? hipMalloc(&d_out, rows.size() * sizeof(float)) : e;
	e = e == hipSuccess ? hipMemcpy(d_in, w.pcm.data(), in_bytes, hipMemcpyHostToDevice) : e;
	int r = 0;
	if (e == hipSuccess) {
		r = ofdmrx_util_survey(h, d_in, w.fmt, 0, w.frames, nfft, (int)S, 0, n_rows, (float *)d_out);
		r = r ? r : ofdmrx_synchronize(h);
		if (r)
			std::fprintf(stderr, "ofdmrx_util_survey: %s\n", ofdmrx_strerror(r));
		else
			e = hipMemcpy(rows.data(), d_out, rows.size() * sizeof(float), hipMemcpyDeviceToHost);
	}
	if (e != hipSuccess)
		std::fprintf(stderr, "survey: %s\n", hipGetErrorString(e));
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	if (r || e != hipSuccess)
		return false;
	std::vector<float> row((size_t)nfft);
	for (size_t i = 0; i < (size_t)nfft; ++i) {
		double sum = 0.0;
		for (size_t k = 0; k < n_rows; ++k)
			sum += (double)rows[k * (size_t)nfft + i];
		row[i] = (float)(sum / (double)n_rows);
	}
	size_t n = 0;
	bands.resize((size_t)nfft);
	r = ofdmrx_util_find_bands(row.data(), nfft, (double)w.rate, SURVEY_THR_DB, SURVEY_GAP_HZ, SURVEY_MIN_WIDTH_HZ, 0.0, bands.size(), bands.data(), &n, &floor);
	if (r) {
		std::fprintf(stderr, "ofdmrx_util_find_bands: %s\n", ofdmrx_strerror(r));
		return false;
	}
	bands.resize(n);
	return true;
}

// ---- what `survey --grid` and `decode_stream --grid DECIM auto[:FLOOR_DB]` share: the occupied slots of a whole grid capture
// (ofdmrx_util_survey_grid + ofdmrx_util_find_slots) with the finder's default parameters.
constexpr double SURVEY_SEP_DB = 8.0;
constexpr int SURVEY_GRID_TIMES = 4096;                           // output times per row

inline bool grid_decim_valid(int d) { return d >= 2 && d <= 512 && !(d & (d - 1)); }

// FLOOR_DB, an absolute floor as 10 log10 of the per-slot power re full scale -> the finder's abs_floor (false: not a number)
static bool survey_floor_arg(const char *arg, double &abs_floor)
{
	char *e = nullptr;
	const double db = std::strtod(arg, &e);
	if (e == arg || *e || !(db > -400.0 && db < 400.0))
		return false;
	abs_floor = std::pow(10.0, db / 10.0);
	return true;
}

// w: a 2-channel capture read by read_wav.  The file is surveyed in blocks of whole rows of 4096 output times, each call given the
// positions its rows need; the per-slot maximum over the rows (peak hold) goes to the finder, so a burst does not vanish in a long
// file's mean.  A trailing partial row is dropped.  abs_floor 0: the median.  Returns false with a message on stderr; slots may come
// back empty.
static bool survey_grid_capture(ofdmrx_handle *h, const Wav &w, int decim, double abs_floor, std::vector<ofdmrx_slot> &slots, double &floor)
{
	const size_t D = (size_t)decim, M = 2 * D, S = SURVEY_GRID_TIMES;
	const size_t times = w.frames ? (w.frames - 1) / D + 1 : 0, n_rows = times / S;
	if (!n_rows) {
		std::fprintf(stderr, "The capture is shorter than one row of %zu output times (%zu samples).\n", S, (S - 1) * D + 1);
		return false;
	}
	const size_t unit = w.pcm.size() / w.frames, per_block = std::max<size_t>(1, 1024 / D);
	const size_t max_in = (per_block * S + 24) * D;
	void *d_in = nullptr, *d_out = nullptr;
	std::vector<float> rows(per_block * M), peak(M, 0.f);
	hipError_t e = hipMalloc(&d_in, max_in * unit);
	e = e == hipSuccess ? hipMalloc(&d_out, rows.size() * sizeof(float)) : e;
	int r = 0;
	for (size_t r0 = 0; r0 < n_rows && e == hipSuccess && !r; r0 += per_block) {
		const size_t nb = std::min(per_block, n_rows - r0);
		const size_t first = r0 * S > 24 ? (r0 * S - 24) * D : 0, count = ((r0 + nb) * S - 1) * D - first + 1;
		e = hipMemcpy(d_in, w.pcm.data() + first * unit, count * unit, hipMemcpyHostToDevice);
		if (e != hipSuccess)
			break;
		r = ofdmrx_util_survey_grid(h, d_in, w.fmt, (long long)first, count, decim, (int)S, (long long)r0, nb, (float *)d_out);
		r = r ? r : ofdmrx_synchronize(h);
		if (r) {
			std::fprintf(stderr, "ofdmrx_util_survey_grid: %s\n", ofdmrx_strerror(r));
			break;
		}
		e = hipMemcpy(rows.data(), d_out, nb * M * sizeof(float), hipMemcpyDeviceToHost);
		for (size_t j = 0; j < nb * M && e == hipSuccess; ++j)
			peak[j % M] = std::max(peak[j % M], rows[j]);
	}
	if (e != hipSuccess)
		std::fprintf(stderr, "survey: %s\n", hipGetErrorString(e));
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	if (r || e != hipSuccess)
		return false;
	size_t n = 0;
	slots.resize(M);
	r = ofdmrx_util_find_slots(peak.data(), decim, (double)w.rate / (double)decim, SURVEY_THR_DB, SURVEY_SEP_DB, abs_floor, slots.size(), slots.data(), &n, &floor);
	if (r) {
		std::fprintf(stderr, "ofdmrx_util_find_slots: %s\n", ofdmrx_strerror(r));
		return false;
	}
	slots.resize(n);
	return true;
}

// ---- the same at a ratio, for `survey --grid-ratio` and `decode_stream --grid-ratio P/Q auto[:FLOOR_DB]` (ofdmrx_util_survey_grid_ratio
// + ofdmrx_util_find_slots_ratio).  p / q: any spelling of a ratio the grid front end at a ratio takes
// (ofdmrx_util_grid_ratio_slots accepts it); w.rate q / p is the handle's rate.  Rows of 4096 output times, peak hold over the rows,
// a trailing partial row dropped, abs_floor 0: the median.
static bool survey_grid_ratio_capture(ofdmrx_handle *h, const Wav &w, int p, int q, double abs_floor, std::vector<ofdmrx_slot> &slots, double &floor)
{
	int32_t k_first = 0;
	size_t N = 0;
	if (p <= 0 || q <= 0 || ofdmrx_util_grid_ratio_slots(p, q, &k_first, &N)) {
		std::fprintf(stderr, "A grid survey at a ratio takes P/Q with, in lowest terms, Q 1 .. 16 and P 2 Q .. 512 with no prime factor other than 2, 3 and 5.\n");
		return false;
	}
	size_t g = (size_t)p, b = (size_t)q;
	while (b) {
		const size_t t = g % b;
		g = b;
		b = t;
	}
	const size_t P = (size_t)p / g, Q = (size_t)q / g, S = SURVEY_GRID_TIMES, H = 24 * P / Q;
	// output time n ends inside the file where (n P) div Q <= frames - 1
	const size_t times = w.frames ? (w.frames * Q - 1) / P + 1 : 0, n_rows = times / S;
	if (!n_rows) {
		std::fprintf(stderr, "The capture is shorter than one row of %zu output times (%zu samples).\n", S, (S - 1) * P / Q + 1);
		return false;
	}
	const size_t unit = w.pcm.size() / w.frames, per_block = std::max<size_t>(1, 1024 * Q / P);
	const size_t max_in = per_block * S * P / Q + H + 2;
	void *d_in = nullptr, *d_out = nullptr;
	std::vector<float> rows(per_block * N), peak(N, 0.f);
	hipError_t e = hipMalloc(&d_in, max_in * unit);
	e = e == hipSuccess ? hipMalloc(&d_out, rows.size() * sizeof(float)) : e;
	int r = 0;
	for (size_t r0 = 0; r0 < n_rows && e == hipSuccess && !r; r0 += per_block) {
		const size_t nb = std::min(per_block, n_rows - r0);
		const size_t at = r0 * S * P / Q, first = at > H ? at - H : 0, count = ((r0 + nb) * S - 1) * P / Q - first + 1;
		e = hipMemcpy(d_in, w.pcm.data() + first * unit, count * unit, hipMemcpyHostToDevice);
		if (e != hipSuccess)
			break;
		r = ofdmrx_util_survey_grid_ratio(h, d_in, w.fmt, (long long)first, count, p, q, (int)S, (long long)r0, nb, (float *)d_out);
		r = r ? r : ofdmrx_synchronize(h);
		if (r) {
			std::fprintf(stderr, "ofdmrx_util_survey_grid_ratio: %s\n", ofdmrx_strerror(r));
			break;
		}
		e = hipMemcpy(rows.data(), d_out, nb * N * sizeof(float), hipMemcpyDeviceToHost);
		for (size_t j = 0; j < nb * N && e == hipSuccess; ++j)
			peak[j % N] = std::max(peak[j % N], rows[j]);
	}
	if (e != hipSuccess)
		std::fprintf(stderr, "survey: %s\n", hipGetErrorString(e));
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	if (r || e != hipSuccess)
		return false;
	size_t n = 0;
	slots.resize(N);
	r = ofdmrx_util_find_slots_ratio(peak.data(), p, q, (double)w.rate * (double)q / (double)p, SURVEY_THR_DB, SURVEY_SEP_DB, abs_floor, slots.size(), slots.data(), &n, &floor);
	if (r) {
		std::fprintf(stderr, "ofdmrx_util_find_slots_ratio: %s\n", ofdmrx_strerror(r));
		return false;
	}
	slots.resize(n);
	return true;
}
