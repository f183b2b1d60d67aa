// k_channelize.hip -- the wideband front end: one wideband I/Q capture -> many receiver channels at the
// handle's rate: mix-down by an integer-phase NCO, a 24 D + 1 tap FIR, decimation by D.  Every output is a closed form of absolute
// sample indices, so the kernel has no state and a capture cuts into blocks without changing a bit.
//   y_c[n] = e^{-2 pi i phi_c(n D) / 2^32} * sum_k (h[k] e^{+2 pi i phi_c(k) / 2^32}) x[n D - k],   phi_c(m) = inc_c m mod 2^32
// One workgroup makes CHZ tile = 64 R outputs of four channels, one wave per channel, lane l the outputs l, l + 64, ... of the tile:
//   the tile's input span (tile - 1 + 24) D + 1 samples is converted once and laid out in LDS by polyphase - sample s of the span at
//   [s mod D][s / D] - so that for a given tap the 64 lanes of a wave read 64 neighbouring float2 (ds_read_b64, no bank conflict) and
//   the tap itself is one broadcast read; each wave forms its channel's modulated taps h[k] e^{+i theta_c(k)} in LDS first.
// The order of the sum is part of the definition's contract: phase b = k mod D ascending, inside it a = k / D ascending, one FMA chain
// per component (re: + g.re x.re, - g.im x.im; im: + g.re x.im, + g.im x.re).  It does not depend on the tile, the launch or the
// block an output belongs to: positions outside [in_first, in_first + n_in) are never loaded and enter as +0.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int CHZ_WAVES = 4;                                      // channels per workgroup
constexpr int CHZ_HIST = 24;                                      // (T - 1) / D: rows of history in front of a tile

// R: outputs per lane; the tile is 64 R outputs, its rows in LDS 64 R + CHZ_HIST, padded to an odd count
template <int FMT, int R>
__global__ __launch_bounds__(64 * CHZ_WAVES) void k_channelize(ChannelizeArgs a)
{
	constexpr int TILE = 64 * R, ROWS = TILE + CHZ_HIST + 1;
	extern __shared__ float2 chz_lds[];
	const int D = a.p, T = 2 * 12 * D + 1;
	float2 *xs = chz_lds;                                         // [D][ROWS]
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	float2 *g = chz_lds + D * ROWS + w * T;                       // [CHZ_WAVES][T]
	const long long n0 = a.out_first + (long long)blockIdx.x * TILE;
	const long long m_lo = (n0 - CHZ_HIST) * D;
	const int span = (TILE - 1 + CHZ_HIST) * D + 1;
	for (int s = tid; s < span; s += 64 * CHZ_WAVES) {
		const long long m = m_lo + s;
		float2 v = make_float2(0.f, 0.f);
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = iq_sample<FMT>(a.in, (size_t)(m - a.in_first));
		const int q = s / D, p = s - q * D;
		xs[p * ROWS + q] = v;
	}
	const int c = (int)blockIdx.y * CHZ_WAVES + w;
	const bool live = c < a.n_channels;
	const unsigned inc = live ? a.inc[c] : 0u;
	for (int k = lane; k < T; k += 64) {
		float cs, sn;
		phase_phasor(inc * (unsigned)k, cs, sn);
		const float h = a.taps[k];
		g[k] = make_float2(h * cs, h * sn);
	}
	__syncthreads();
	if (!live)
		return;
	float re[R], im[R];
	#pragma unroll
	for (int r = 0; r < R; ++r)
		re[r] = im[r] = 0.f;
	// tap k = a D + b meets output row j at span sample (j + 24 - a) D - b: plane 0, row j + 24 - a for b = 0, else plane D - b, row j + 23 - a
	for (int b = 0; b < D; ++b) {
		const float2 *xp = xs + (b ? D - b : 0) * ROWS + (b ? CHZ_HIST - 1 : CHZ_HIST) + lane;
		const float2 *gp = g + b;
		const int na = b ? CHZ_HIST : CHZ_HIST + 1;
		for (int i = 0; i < na; ++i) {
			const float2 t = gp[i * D];
			#pragma unroll
			for (int r = 0; r < R; ++r) {
				const float2 x = xp[64 * r - i];
				re[r] = __builtin_fmaf(t.x, x.x, re[r]);
				re[r] = __builtin_fmaf(-t.y, x.y, re[r]);
				im[r] = __builtin_fmaf(t.x, x.y, im[r]);
				im[r] = __builtin_fmaf(t.y, x.x, im[r]);
			}
		}
	}
	float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
	#pragma unroll
	for (int r = 0; r < R; ++r) {
		const long long j = (long long)blockIdx.x * TILE + lane + 64 * r;   // the output's place in its row
		if (j >= a.n_out)
			continue;
		float cs, sn;
		phase_phasor(inc * (unsigned)(unsigned long long)((a.out_first + j) * D), cs, sn);
		const float yr = __builtin_fmaf(re[r], cs, im[r] * sn), yi = __builtin_fmaf(im[r], cs, -(re[r] * sn));
		dst[j] = make_float2(yr, yi);
	}
}

template <int FMT> static void chz_launch(hipStream_t s, const ChannelizeArgs &a)
{
	const int D = a.p, T = 24 * D + 1;
	const unsigned groups = (unsigned)((a.n_channels + CHZ_WAVES - 1) / CHZ_WAVES);
	// (64 KiB of LDS hold a tile of 256 outputs up to D = 16, one of 128 above: 48288 bytes at D = 16, 63776 at D = 32)
	if (D <= 16) {
		constexpr int R = 4;
		const size_t lds = ((size_t)D * (64 * R + CHZ_HIST + 1) + (size_t)CHZ_WAVES * T) * sizeof(float2);
		hipLaunchKernelGGL((k_channelize<FMT, R>), dim3((unsigned)((a.n_out + 64 * R - 1) / (64 * R)), groups), dim3(64 * CHZ_WAVES), lds, s, a);
	} else {
		constexpr int R = 2;
		const size_t lds = ((size_t)D * (64 * R + CHZ_HIST + 1) + (size_t)CHZ_WAVES * T) * sizeof(float2);
		hipLaunchKernelGGL((k_channelize<FMT, R>), dim3((unsigned)((a.n_out + 64 * R - 1) / (64 * R)), groups), dim3(64 * CHZ_WAVES), lds, s, a);
	}
}

// (k_channelize's shortest tile is 128 outputs, k_rechannelize's 32: the grid's x stays below 2^31)
long long channelize_max_outputs(int q) { return (q == 1 ? 128LL : 32LL) * 0x7fffffffLL; }

void launch_channelize(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.q != 1)
		launch_channelize_ratio(s, a);
	else if (a.fmt == 0)
		chz_launch<0>(s, a);
	else if (a.fmt == 1)
		chz_launch<1>(s, a);
	else
		chz_launch<2>(s, a);
}

}  // namespace rx
