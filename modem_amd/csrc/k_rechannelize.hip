// k_rechannelize.hip -- the wideband front end at a rational decimation P / Q: one wideband I/Q capture ->
// many receiver channels at the handle's rate, rate = Rw Q / P.  Like k_channelize every output is a closed form of absolute sample
// indices: no state, and a capture cuts into blocks without changing a bit.
//   u_n = n P,  i_n = u_n div Q,  q_n = u_n mod Q,   phi_c(m) = inc_c m mod 2^32
//   y_c[n] = e^{-2 pi i phi_c(i_n) / 2^32} * sum_j (h_{q_n}[j] e^{+2 pi i phi_c(j) / 2^32}) x[i_n - j],   j = 0 .. T - 1
// Because gcd(P, Q) = 1 the outputs n = rho (mod Q) share one phase q and their inputs lie exactly P apart: Q interleaved decimators
// by the integer P.  A workgroup makes one TILE = Q M outputs (tiles are cut at ABSOLUTE multiples of Q M, so that a tile begins on
// residue 0) of four channels, one wave per channel.  Slot e = rho M + m of a tile is output n = tile Q M + rho + Q m; lane l takes the
// slots l, l + 64, ... (NP of them: rechannelize_shape picks M and NP so that few of the 64 NP slots stay empty).  The tile's input
// span (M + H) P samples, H = ceil((T - 1) / P) rows of history, is converted
// once and laid out in LDS by polyphase of P - sample s of the span at [s mod P][s / P] - so the M lanes of one residue read M
// neighbouring float2 for a given tap.  The taps lie in device memory as [T][Q]: for a given j every lane of a wave reads inside one
// 64-byte line; the wave's phasors e^{+i phi_c(j)} lie in LDS (one broadcast read per tap).
// The order of the sum is part of the definition's contract: j ascending, one FMA chain per component (re: + g.re x.re, - g.im x.im;
// im: + g.re x.im, + g.im x.re), g = (fl(h cos), fl(h sin)).  It does not depend on the tile, the launch, the block or the residue
// grouping: positions outside [in_first, in_first + n_in) are never loaded and enter as +0.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int RCZ_WAVES = 4;                                      // channels per workgroup
constexpr int RCZ_R = 4;                                          // slots per lane at most: a tile has at most 256
constexpr size_t RCZ_LDS = 65536;                                 // the span and the phasors stay inside it: two workgroups per CU

// the tile's shape, from rechannelize_shape: T, M, the rows of history, the rows of a plane in LDS
struct RczTile { int n_taps, m, hist, rows; };

template <int FMT, int NP>
__global__ __launch_bounds__(64 * RCZ_WAVES) void k_rechannelize(ChannelizeArgs a, RczTile g)
{
	extern __shared__ float2 rcz_lds[];
	const int P = a.p, Q = a.q, T = g.n_taps, M = g.m, H = g.hist, ROWS = g.rows;
	float2 *xs = rcz_lds;                                         // [P][ROWS]
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	float2 *ph = rcz_lds + P * ROWS + w * T;                      // [RCZ_WAVES][T]
	const int tile = Q * M;
	const long long t = a.out_first / tile + (long long)blockIdx.x;   // the tile, counted from output 0
	const long long m_lo = (t * M - H) * P;                       // i_n of the tile's first output is t M P
	const int span = (M + H) * P;
	for (int s = tid; s < span; s += 64 * RCZ_WAVES) {
		const long long m = m_lo + s;
		float2 v = make_float2(0.f, 0.f);
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = iq_sample<FMT>(a.in, (size_t)(m - a.in_first));
		const int row = s / P, pl = s - row * P;
		xs[pl * ROWS + row] = v;
	}
	const int c = (int)blockIdx.y * RCZ_WAVES + w;
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
			const float2 x = xs[at[r]];
			re[r] = __builtin_fmaf(gx, x.x, re[r]);
			re[r] = __builtin_fmaf(-gy, x.y, re[r]);
			im[r] = __builtin_fmaf(gx, x.y, im[r]);
			im[r] = __builtin_fmaf(gy, x.x, im[r]);
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
		dst[j] = make_float2(yr, yi);
	}
}

// M outputs per residue and tile: as many as leave the span [P][(M + H) | 1] and the four waves' phasors inside RCZ_LDS (the fewest
// are 7, at 511/16: 9 rows of 511 samples and 4 x 767 phasors are 61336 bytes), and at most 64 NP / Q for NP slots per lane; NP is
// the largest of 4 .. 1 at which 85 % of the 64 NP slots hold an output (NP = 1 fills them all but for Q M < 64)
RechannelizeShape rechannelize_shape(int p, int q)
{
	RechannelizeShape g{};
	g.n_taps = 24 * p / q + 1;
	g.hist = (g.n_taps - 1 + p - 1) / p;
	int rows = (int)((RCZ_LDS - (size_t)RCZ_WAVES * (size_t)g.n_taps * sizeof(float2)) / sizeof(float2) / (size_t)p);
	if (rows % 2 == 0)
		rows -= 1;
	const int m_lds = rows - g.hist;
	for (g.passes = RCZ_R; g.passes >= 1; --g.passes) {
		g.m = std::min(64 * g.passes / q, m_lds);
		if (100 * q * g.m >= 85 * 64 * g.passes || g.passes == 1)
			break;
	}
	g.rows = (g.m + g.hist) | 1;
	g.lds = ((size_t)p * (size_t)g.rows + (size_t)RCZ_WAVES * (size_t)g.n_taps) * sizeof(float2);
	return g;
}

template <int FMT, int NP> static void rcz_launch_np(hipStream_t s, const ChannelizeArgs &a, const RechannelizeShape &g)
{
	const long long tile = (long long)a.q * g.m;
	const long long tiles = (a.out_first + a.n_out - 1) / tile - a.out_first / tile + 1;
	const unsigned groups = (unsigned)((a.n_channels + RCZ_WAVES - 1) / RCZ_WAVES);
	const RczTile t{ g.n_taps, g.m, g.hist, g.rows };
	hipLaunchKernelGGL((k_rechannelize<FMT, NP>), dim3((unsigned)tiles, groups), dim3(64 * RCZ_WAVES), g.lds, s, a, t);
}

template <int FMT> static void rcz_launch_fmt(hipStream_t s, const ChannelizeArgs &a)
{
	const RechannelizeShape g = rechannelize_shape(a.p, a.q);
	if (g.passes == 4)
		rcz_launch_np<FMT, 4>(s, a, g);
	else if (g.passes == 3)
		rcz_launch_np<FMT, 3>(s, a, g);
	else if (g.passes == 2)
		rcz_launch_np<FMT, 2>(s, a, g);
	else
		rcz_launch_np<FMT, 1>(s, a, g);
}

void launch_channelize_ratio(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.fmt == 0)
		rcz_launch_fmt<0>(s, a);
	else if (a.fmt == 1)
		rcz_launch_fmt<1>(s, a);
	else
		rcz_launch_fmt<2>(s, a);
}

}  // namespace rx
