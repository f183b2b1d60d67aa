// k_survey.hip -- the wideband survey: an averaged (Welch) power spectrum of one wideband I/Q capture, as
// one row or as a waterfall of rows.  Every output is a closed form of absolute sample indices, so the kernel has no state and a
// capture surveyed row by row gives the same bytes as one call.
//   segment s: positions s H .. s H + N - 1, H = N / 2;   X_s[b] = sum_n w[n] x[s H + n] e^{-2 pi i b n / N}, w = periodic Hann (fp32)
//   row r, S = segs_per_row:   P[r][i] = (1 / (S U)) sum_{s = r S .. r S + S - 1} |X_s[(i + N / 2) mod N]|^2,   U = sum w^2
// k_survey: one workgroup per (row, group of SURVEY_G consecutive segments counted from the row's first).  The hop is N / 2, so
// every sample belongs to two segments: the half a segment shares with the next one is converted once and stays in LDS; the new
// half of the NEXT segment is loaded while this one is transformed.  The window is multiplied in on the way into the transform's
// buffer, the transform runs in LDS with the plan's compact twiddles (dev_common.h: FftPlan), and every thread keeps |X|^2 of its
// N / NT bins in registers over the group's segments.  The partial goes out in natural bin order with coalesced stores.
// k_survey_rows: sums a row's partials in ascending group order, scales, and writes the row shifted to ascending frequency.
// The order of the sum is part of the definition's contract and depends on absolute indices only: |X|^2 = fma(im, im, re re), one
// fp32 chain over the segments of a group in ascending order, then one fp32 chain over the groups in ascending order, one product
// with fp32(1 / (S U)).  No float atomics, no "last workgroup finishes".
// LDS layout, by argument: thread t touches elements t + NT k (8-byte cf) of the buffer and of the shared half - 64 lanes, 64
// consecutive 8-byte words, one ds_write_b64 / ds_read_b64 each at the 64-dword bank modulus: no bank conflict on the load side.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

template <int N> struct SurveyCfg {
	static constexpr int NT = N == 1280 ? 320 : 640;              // every radix-4 stage of 1280 is one butterfly per thread; 2 at 2560 / 5120 (4 at 5120's)
	static constexpr int H = N / 2;
	static_assert(H % NT == 0, "a thread owns whole columns of the half segment");
};

template <int FMT> __device__ __forceinline__ cf survey_sample(const SurveyArgs &a, long long m)
{
	const long long i = m - a.in_first;
	if (i < 0 || i >= a.n_in)                                     // (the host refuses such a call: never taken)
		return mk(0.f, 0.f);
	const float2 v = iq_sample<FMT>(a.in, (size_t)i);
	return mk(v.x, v.y);
}

template <int FMT, int N>
__global__ __launch_bounds__(SurveyCfg<N>::NT) void k_survey(SurveyArgs a)
{
	constexpr int NT = SurveyCfg<N>::NT, H = N / 2, KH = H / NT, KN = N / NT;
	__shared__ cf buf[N];
	__shared__ cf half[H];
	__shared__ cf twc[fft_compact_size<N, N>()];
	const int tid = threadIdx.x;
	const long long r_local = (long long)blockIdx.x / a.n_groups;
	const int g = (int)((long long)blockIdx.x - r_local * a.n_groups);
	const int n_seg = min(SURVEY_G, a.segs_per_row - g * SURVEY_G);
	const long long s0 = (a.row_first + r_local) * a.segs_per_row + (long long)g * SURVEY_G;
	fft_compact_twiddles<N, NT, N>(twc, a.tw, tid);
	float w[KN], acc[KN];
	#pragma unroll
	for (int k = 0; k < KN; ++k) {
		w[k] = a.win[tid + NT * k];
		acc[k] = 0.f;
	}
	cf nxt[KH];
	#pragma unroll
	for (int k = 0; k < KH; ++k) {
		half[tid + NT * k] = survey_sample<FMT>(a, s0 * H + tid + NT * k);
		nxt[k] = survey_sample<FMT>(a, (s0 + 1) * H + tid + NT * k);
	}
	for (int j = 0; j < n_seg; ++j) {
		#pragma unroll
		for (int k = 0; k < KH; ++k) {                            // (half[] is private to its thread: no barrier around it)
			const int n = tid + NT * k;
			const cf x = half[n], y = nxt[k];
			buf[n] = mk(w[k] * x.re, w[k] * x.im);
			buf[H + n] = mk(w[KH + k] * y.re, w[KH + k] * y.im);
			half[n] = y;
		}
		if (j + 1 < n_seg) {
			#pragma unroll
			for (int k = 0; k < KH; ++k)
				nxt[k] = survey_sample<FMT>(a, (s0 + j + 2) * H + tid + NT * k);
		}
		__syncthreads();
		fft_fwd_compact<N, NT, N>(buf, twc, tid);
		#pragma unroll
		for (int k = 0; k < KN; ++k) {
			const cf X = buf[tid + NT * k];
			acc[k] += __builtin_fmaf(X.im, X.im, X.re * X.re);
		}
		__syncthreads();
	}
	float *dst = a.part + (size_t)blockIdx.x * N;
	#pragma unroll
	for (int k = 0; k < KN; ++k)
		dst[tid + NT * k] = acc[k];
}

__global__ __launch_bounds__(256) void k_survey_rows(SurveyArgs a, float scale)
{
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
	const int N = a.nfft;
	if (t >= a.n_rows * N)
		return;
	const long long r = t / N;
	const int i = (int)(t - r * N);
	const int b = i + N / 2 < N ? i + N / 2 : i - N / 2;
	const float *p = a.part + (size_t)r * (size_t)a.n_groups * N + b;
	// the same ordered chain, eight loads in flight at a time (one load per addition waited a memory round trip per group)
	float s = p[0];
	int g = 1;
	for (; g + 8 <= a.n_groups; g += 8) {
		float v[8];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			v[j] = p[(size_t)(g + j) * N];
		#pragma unroll
		for (int j = 0; j < 8; ++j)
			s += v[j];
	}
	for (; g < a.n_groups; ++g)
		s += p[(size_t)g * N];
	a.out[t] = s * scale;
}

template <int N> static void survey_launch(hipStream_t s, const SurveyArgs &a)
{
	const dim3 grid((unsigned)(a.n_rows * a.n_groups)), block(SurveyCfg<N>::NT);
	if (a.fmt == 0)
		hipLaunchKernelGGL((k_survey<0, N>), grid, block, 0, s, a);
	else if (a.fmt == 1)
		hipLaunchKernelGGL((k_survey<1, N>), grid, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_survey<2, N>), grid, block, 0, s, a);
}

void launch_survey(hipStream_t s, const SurveyArgs &a, float scale)
{
	if (a.nfft == 1280)
		survey_launch<1280>(s, a);
	else if (a.nfft == 2560)
		survey_launch<2560>(s, a);
	else
		survey_launch<5120>(s, a);
	hipLaunchKernelGGL(k_survey_rows, dim3((unsigned)((a.n_rows * a.nfft + 255) / 256)), dim3(256), 0, s, a, scale);
}

}  // namespace rx
