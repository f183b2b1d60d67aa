// survey_cli.h -- what `survey` and `decode_stream --wideband DECIM|P/Q auto` share: the decimation argument, and the occupied bands
// of a whole wideband capture
// (ofdmrx_util_survey + ofdmrx_util_find_bands) with the finder's default parameters.
#pragma once
#include "wav_read.h"
#include <hip/hip_runtime.h>
#include <algorithm>
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
