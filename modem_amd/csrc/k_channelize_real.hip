// k_channelize_real.hip -- the wideband front end for a REAL capture: one value per wideband position ->
// many receiver channels at the handle's rate, at the integer decimation D (k_channelize_real, section 4.14's form) or at the ratio
// P / Q (k_rechannelize_real, section 4.17's form).  For a real x the mix-down and low-pass is itself the Hilbert step - the stop band
// removes the mirror image - so this is 4.14 / 4.17 on the capture (x, +0) with the products by the zero component left out and the
// result doubled: the same taps, increments, output times and summation order,
//   y_c[n] = 2 e^{-2 pi i phi_c(i_n) / 2^32} * sum_j (h_{q_n}[j] e^{+2 pi i phi_c(j) / 2^32}) x[i_n - j],   phi_c(m) = inc_c m mod 2^32
// one FMA chain per component (re += g.re x, im += g.im x, g = (fl(h cos), fl(h sin))), the output rotation as k_channelize and
// k_rechannelize write it, the multiplication by 2.0f last (exact).  Adding -g.im * (+0) to a chain that starts at +0 never changes
// a bit, so the outputs are, byte for byte, twice what those kernels give for the same samples with a +0 imaginary part.
// The organisation is theirs - one wave per channel, lane l the outputs (slots) l, l + 64, ..., the span laid out by polyphase in
// LDS - with the span as float: for a given tap the 64 lanes of a wave read 64 neighbouring floats (ds_read_b32, no bank conflict
// whatever the padding), and the span costs half the LDS.  The modulated taps (the phasors) stay float2 per wave and lie in front of
// the span, on their 8-byte boundary.  Positions outside [in_first, in_first + n_in) are never loaded and enter as +0.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int CHR_WAVES = 4;                                      // channels per workgroup
constexpr int CHR_HIST = 24;                                      // (T - 1) / D: rows of history in front of a tile
constexpr int CHR_R = 4;                                          // outputs per lane: a tile of 256 at every D (see chr_launch)
constexpr size_t CHR_LDS = 65536;                                 // the phasors and the span stay inside it

// value i of a one-channel capture as fp32, scaled as iq_sample scales a component; FMT: 0 S16, 1 U8, 2 F32.  The caller has checked
// the bounds
template <int FMT> __device__ __forceinline__ float real_sample(const void *in, size_t i)
{
	if (FMT == 0)
		return div_32767((float)((const short *)in)[i]);
	if (FMT == 1)
		return div_127((float)((int)((const uint8_t *)in)[i] - 128));
	return ((const float *)in)[i];
}

// the tile is 64 R outputs, its rows in LDS 64 R + CHR_HIST, padded to an odd count
template <int FMT, int R>
__global__ __launch_bounds__(64 * CHR_WAVES) void k_channelize_real(ChannelizeArgs a)
{
	constexpr int TILE = 64 * R, ROWS = TILE + CHR_HIST + 1;
	extern __shared__ float2 chr_lds[];
	const int D = a.p, T = 2 * 12 * D + 1;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	float2 *g = chr_lds + w * T;                                  // [CHR_WAVES][T]
	float *xs = (float *)(chr_lds + CHR_WAVES * T);               // [D][ROWS]
	const long long n0 = a.out_first + (long long)blockIdx.x * TILE;
	const long long m_lo = (n0 - CHR_HIST) * D;
	const int span = (TILE - 1 + CHR_HIST) * D + 1;
	for (int s = tid; s < span; s += 64 * CHR_WAVES) {
		const long long m = m_lo + s;
		float v = 0.f;
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = real_sample<FMT>(a.in, (size_t)(m - a.in_first));
		const int q = s / D, p = s - q * D;
		xs[p * ROWS + q] = v;
	}
	const int c = (int)blockIdx.y * CHR_WAVES + w;
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
		const float *xp = xs + (b ? D - b : 0) * ROWS + (b ? CHR_HIST - 1 : CHR_HIST) + lane;
		const float2 *gp = g + b;
		const int na = b ? CHR_HIST : CHR_HIST + 1;
		for (int i = 0; i < na; ++i) {
			const float2 t = gp[i * D];
			#pragma unroll
			for (int r = 0; r < R; ++r) {
				const float x = xp[64 * r - i];
				re[r] = __builtin_fmaf(t.x, x, re[r]);
				im[r] = __builtin_fmaf(t.y, x, im[r]);
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
		dst[j] = make_float2(2.0f * yr, 2.0f * yi);
	}
}

// The outputs per lane from the LDS budget: a tile of 64 R outputs costs 8 x 4 (24 D + 1) bytes of modulated taps and 4 D (64 R + 25)
// bytes of span.  R = 4: 1892 D + 32 bytes - 3816 at D = 2, 30304 at D = 16, 60576 at D = 32, inside 64 KiB at every D, so the launch
// has ONE shape (k_channelize falls back to R = 2 above D = 16; here nothing changes there).  R = 8 would fit up to D = 22 only
// (2916 D + 32 bytes) and is not taken: it halves the workgroups of a bank's push, which has few, and would bring the change of shape back.
template <int FMT> static void chr_launch(hipStream_t s, const ChannelizeArgs &a)
{
	constexpr int R = CHR_R;
	const int D = a.p, T = 24 * D + 1;
	const unsigned groups = (unsigned)((a.n_channels + CHR_WAVES - 1) / CHR_WAVES);
	const size_t lds = (size_t)CHR_WAVES * T * sizeof(float2) + (size_t)D * (64 * R + CHR_HIST + 1) * sizeof(float);
	static_assert((size_t)CHR_WAVES * (24 * 32 + 1) * sizeof(float2) + (size_t)32 * (64 * R + CHR_HIST + 1) * sizeof(float) <= CHR_LDS, "D = 32 must fit");
	hipLaunchKernelGGL((k_channelize_real<FMT, R>), dim3((unsigned)((a.n_out + 64 * R - 1) / (64 * R)), groups), dim3(64 * CHR_WAVES), lds, s, a);
}

// the tile's shape, from rechannelize_real_shape: T, M, the rows of history, the rows of a plane in LDS
struct RcrTile { int n_taps, m, hist, rows; };

// k_rechannelize's form: Q interleaved decimators by P, tiles cut at ABSOLUTE multiples of Q M, slot e = rho M + m of a tile is output
// n = tile Q M + rho + Q m, lane l the slots l, l + 64, ... (NP of them); the taps [T][Q] in device memory, the phasors in LDS
template <int FMT, int NP>
__global__ __launch_bounds__(64 * CHR_WAVES) void k_rechannelize_real(ChannelizeArgs a, RcrTile g)
{
	extern __shared__ float2 rcr_lds[];
	const int P = a.p, Q = a.q, T = g.n_taps, M = g.m, H = g.hist, ROWS = g.rows;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	float2 *ph = rcr_lds + w * T;                                 // [CHR_WAVES][T]
	float *xs = (float *)(rcr_lds + CHR_WAVES * T);               // [P][ROWS]
	const int tile = Q * M;
	const long long t = a.out_first / tile + (long long)blockIdx.x;   // the tile, counted from output 0
	const long long m_lo = (t * M - H) * P;                       // i_n of the tile's first output is t M P
	const int span = (M + H) * P;
	for (int s = tid; s < span; s += 64 * CHR_WAVES) {
		const long long m = m_lo + s;
		float v = 0.f;
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = real_sample<FMT>(a.in, (size_t)(m - a.in_first));
		const int row = s / P, pl = s - row * P;
		xs[pl * ROWS + row] = v;
	}
	const int c = (int)blockIdx.y * CHR_WAVES + w;
	const bool live = c < a.n_channels;
	const unsigned inc = live ? a.inc[c] : 0u;
	for (int j = lane; j < T; j += 64) {
		float cs, sn;
		phase_phasor(inc * (unsigned)j, cs, sn);
		ph[j] = make_float2(cs, sn);
	}
	__syncthreads();
	if (!live)
		return;
	// slot e: residue rho = e / M, m = e % M; i_n = t M P + o + m P with o = rho P div Q, q = rho P mod Q.  Tap j meets span sample
	// v = H P + o + m P - j >= 0: plane v mod P, row v / P.  A slot outside the tile works on slot 0's places and stores nothing.
	float re[NP], im[NP];
	unsigned at[NP];
	int q[NP];
	long long n_of[NP];
	#pragma unroll
	for (int r = 0; r < NP; ++r) {
		const int e = lane + 64 * r;
		const bool in_tile = e < tile;
		const int rho = in_tile ? e / M : 0, m = in_tile ? e - rho * M : 0;
		const int o = rho * P / Q;
		q[r] = rho * P - o * Q;
		at[r] = (unsigned)(o * ROWS + H + m);                         // v = H P + o: plane o, row H
		n_of[r] = in_tile ? t * tile + rho + (long long)Q * m : -1;
		re[r] = im[r] = 0.f;
	}
	const unsigned wrap = (unsigned)(P * ROWS - 1);
	const float *hp = a.taps;
	for (int j = 0; j < T; ++j, hp += Q) {
		const float2 f = ph[j];
		#pragma unroll
		for (int r = 0; r < NP; ++r) {
			const float h = hp[q[r]];
			const float gx = h * f.x, gy = h * f.y;
			const float x = xs[at[r]];
			re[r] = __builtin_fmaf(gx, x, re[r]);
			im[r] = __builtin_fmaf(gy, x, im[r]);
			// the sample before: one plane down; from plane 0 (at < ROWS: the difference wraps round 2^32) to plane P - 1 of the row before
			const unsigned down = at[r] - (unsigned)ROWS;
			at[r] = min(down, down + wrap);
		}
	}
	float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
	#pragma unroll
	for (int r = 0; r < NP; ++r) {
		const long long j = n_of[r] - a.out_first;                    // the output's place in its row
		if (n_of[r] < 0 || j < 0 || j >= a.n_out)
			continue;
		const unsigned long long i_n = (unsigned long long)(n_of[r] * P) / (unsigned)Q;
		float cs, sn;
		phase_phasor(inc * (unsigned)i_n, cs, sn);
		const float yr = __builtin_fmaf(re[r], cs, im[r] * sn), yi = __builtin_fmaf(im[r], cs, -(re[r] * sn));
		dst[j] = make_float2(2.0f * yr, 2.0f * yi);
	}
}

// rechannelize_shape's rule for a span of float: M outputs per residue and tile, as many as leave the four waves' phasors and the span
// [P][(M + H) | 1] of FLOAT inside CHR_LDS (twice the rows of the analytic kernel's span), and at most 64 NP / Q for NP slots per
// lane; NP is the largest of 4 .. 1 at which 85 % of the 64 NP slots hold an output.  The rows no longer bind anywhere: at 511/16,
// where the analytic kernel has 7 outputs per residue, 19 rows leave 17 and the tile is 16 x 16 = 256
RechannelizeShape rechannelize_real_shape(int p, int q)
{
	RechannelizeShape g{};
	g.n_taps = 24 * p / q + 1;
	g.hist = (g.n_taps - 1 + p - 1) / p;
	int rows = (int)((CHR_LDS - (size_t)CHR_WAVES * (size_t)g.n_taps * sizeof(float2)) / sizeof(float) / (size_t)p);
	if (rows % 2 == 0)
		rows -= 1;
	const int m_lds = rows - g.hist;
	for (g.passes = 4; g.passes >= 1; --g.passes) {
		g.m = std::min(64 * g.passes / q, m_lds);
		if (100 * q * g.m >= 85 * 64 * g.passes || g.passes == 1)
			break;
	}
	g.rows = (g.m + g.hist) | 1;
	g.lds = (size_t)CHR_WAVES * (size_t)g.n_taps * sizeof(float2) + (size_t)p * (size_t)g.rows * sizeof(float);
	return g;
}

template <int FMT, int NP> static void rcr_launch_np(hipStream_t s, const ChannelizeArgs &a, const RechannelizeShape &g)
{
	const long long tile = (long long)a.q * g.m;
	const long long tiles = (a.out_first + a.n_out - 1) / tile - a.out_first / tile + 1;
	const unsigned groups = (unsigned)((a.n_channels + CHR_WAVES - 1) / CHR_WAVES);
	const RcrTile t{ g.n_taps, g.m, g.hist, g.rows };
	hipLaunchKernelGGL((k_rechannelize_real<FMT, NP>), dim3((unsigned)tiles, groups), dim3(64 * CHR_WAVES), g.lds, s, a, t);
}

template <int FMT> static void rcr_launch_fmt(hipStream_t s, const ChannelizeArgs &a)
{
	const RechannelizeShape g = rechannelize_real_shape(a.p, a.q);
	if (g.passes == 4)
		rcr_launch_np<FMT, 4>(s, a, g);
	else if (g.passes == 3)
		rcr_launch_np<FMT, 3>(s, a, g);
	else if (g.passes == 2)
		rcr_launch_np<FMT, 2>(s, a, g);
	else
		rcr_launch_np<FMT, 1>(s, a, g);
}

template <int FMT> static void chr_launch_any(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.q == 1)
		chr_launch<FMT>(s, a);
	else
		rcr_launch_fmt<FMT>(s, a);
}

void launch_channelize_real(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.fmt == 0)
		chr_launch_any<0>(s, a);
	else if (a.fmt == 1)
		chr_launch_any<1>(s, a);
	else
		chr_launch_any<2>(s, a);
}

}  // namespace rx
