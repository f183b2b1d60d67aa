// k_channelize.hip -- the wideband front end (DESIGN.md sections 4.14, 4.17, 4.25): one wideband capture -> many receiver channels at
// the handle's rate: mix-down by an integer-phase NCO, a low-pass FIR, decimation by P / Q.  Every output is a closed form of
// absolute sample indices, so the kernels have no state and a capture cuts into blocks without changing a bit.
//   u_n = n P,  i_n = u_n div Q,  q_n = u_n mod Q,   phi_c(m) = inc_c m mod 2^32,   T = 24 P div Q + 1
//   y_c[n] = e^{-2 pi i phi_c(i_n) / 2^32} * sum_j (h_{q_n}[j] e^{+2 pi i phi_c(j) / 2^32}) x[i_n - j],   j = 0 .. T - 1
// Positions outside [in_first, in_first + n_in) are never loaded and enter as +0.  Both kernels give a workgroup one tile of outputs
// of four channels, one wave per channel, lane l the outputs (slots) l, l + 64, ... of the tile; the tile's input span is converted
// once and laid out in LDS by polyphase of P - sample s of the span at [s mod P][s / P], the rows padded to an odd count - so that for
// a given tap the lanes of a wave read neighbouring samples, and the wave's phasors e^{+i phi_c(j)} lie in LDS too (one broadcast
// read per tap; k_channelize keeps them multiplied by the taps).  The order of the sum is part of the definition's contract: one FMA chain per component (re: + g.re x.re,
// - g.im x.im; im: + g.re x.im, + g.im x.re), g = (fl(h cos), fl(h sin)), in the order each form names.  It does not depend on the
// tile, the launch, the block or the grouping an output belongs to.
// k_channelize (4.14), Q = 1, D = P: a tile is 64 R outputs counted from out_first, the span (64 R - 1 + 24) D + 1 samples; each wave
//   forms its channel's modulated taps g in LDS first.  The order: phase b = k mod D ascending, inside it a = k / D ascending.
// k_rechannelize (4.17), Q > 1: because gcd(P, Q) = 1 the outputs n = rho (mod Q) share one phase q and their inputs lie exactly P
//   apart: Q interleaved decimators by the integer P.  A tile is Q M outputs, cut at ABSOLUTE multiples of Q M so that it begins on
//   residue 0; slot e = rho M + m of a tile is output n = tile Q M + rho + Q m, and a lane has NP slots (rechannelize_shape picks M
//   and NP so that few of the 64 NP slots stay empty).  The span is (M + H) P samples, H = ceil((T - 1) / P) rows of history.  The
//   taps lie in device memory as [T][Q]: for a given j every lane of a wave reads inside one 64-byte line.  The order: j ascending.
// A REAL capture (4.25) is a restriction of both, not a third form.  For a real x the mix-down and low-pass is itself the Hilbert
//   step - the stop band removes the mirror image - so it is the sum above on the capture (x, +0) with the products by the zero
//   component left out and the result doubled last (exact): the same taps, increments, output times and order.  Adding
//   -g.im * (+0) to a chain that starts at +0 never changes a bit, so the outputs are, byte for byte, twice the analytic ones.  The
//   span is float - ds_read_b32 for a tap, no bank conflict whatever the padding, half the LDS - and lies behind the phasors, on
//   their 8-byte boundary; an analytic span lies in front of them.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int CHZ_WAVES = 4;                                      // channels per workgroup
constexpr int CHZ_HIST = 24;                                      // k_channelize: (T - 1) / D rows of history in front of a tile
constexpr int CHZ_SLOTS = 4;                                      // outputs (slots) per lane at most: a tile has at most 256
constexpr size_t CHZ_LDS = 65536;                                 // the span and the phasors stay inside it

// what the two kinds of capture differ in: the span's element, its place in LDS, the products of a tap, the doubling
template <bool REAL> struct Capture;
template <> struct Capture<false> {
	using sample = float2;
	static constexpr bool span_first = true;
	static __device__ __forceinline__ sample zero() { return make_float2(0.f, 0.f); }
	template <int FMT> static __device__ __forceinline__ sample load(const void *in, size_t i) { return iq_sample<FMT>(in, i); }
	static __device__ __forceinline__ void mac(float &re, float &im, float gx, float gy, sample x)
	{
		re = __builtin_fmaf(gx, x.x, re);
		re = __builtin_fmaf(-gy, x.y, re);
		im = __builtin_fmaf(gx, x.y, im);
		im = __builtin_fmaf(gy, x.x, im);
	}
	static __device__ __forceinline__ float2 out(float yr, float yi) { return make_float2(yr, yi); }
};
template <> struct Capture<true> {
	using sample = float;
	static constexpr bool span_first = false;
	static __device__ __forceinline__ sample zero() { return 0.f; }
	template <int FMT> static __device__ __forceinline__ sample load(const void *in, size_t i) { return real_sample<FMT>(in, i); }
	static __device__ __forceinline__ void mac(float &re, float &im, float gx, float gy, sample x)
	{
		re = __builtin_fmaf(gx, x, re);
		im = __builtin_fmaf(gy, x, im);
	}
	static __device__ __forceinline__ float2 out(float yr, float yi) { return make_float2(2.0f * yr, 2.0f * yi); }
};

// the accumulated sum of an output, rotated by e^{-i phase}
template <bool REAL> __device__ __forceinline__ float2 rotated(float re, float im, unsigned phase)
{
	float cs, sn;
	phase_phasor(phase, cs, sn);
	const float yr = __builtin_fmaf(re, cs, im * sn), yi = __builtin_fmaf(im, cs, -(re * sn));
	return Capture<REAL>::out(yr, yi);
}

// R: outputs per lane; the tile is 64 R outputs, its rows in LDS 64 R + CHZ_HIST, padded to an odd count
template <bool REAL, int FMT, int R>
__global__ __launch_bounds__(64 * CHZ_WAVES) void k_channelize(ChannelizeArgs a)
{
	using K = Capture<REAL>;
	using X = typename K::sample;
	constexpr int TILE = 64 * R, ROWS = TILE + CHZ_HIST + 1;
	extern __shared__ float2 chz_lds[];
	const int D = a.p, T = 2 * 12 * D + 1;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	X *xs = K::span_first ? (X *)chz_lds : (X *)(chz_lds + CHZ_WAVES * T);            // [D][ROWS]
	float2 *g = (K::span_first ? chz_lds + D * ROWS : chz_lds) + w * T;               // [CHZ_WAVES][T]
	const long long n0 = a.out_first + (long long)blockIdx.x * TILE;
	const long long m_lo = (n0 - CHZ_HIST) * D;
	const int span = (TILE - 1 + CHZ_HIST) * D + 1;
	for (int s = tid; s < span; s += 64 * CHZ_WAVES) {
		const long long m = m_lo + s;
		X v = K::zero();
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = K::template load<FMT>(a.in, (size_t)(m - a.in_first));
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
		const X *xp = xs + (b ? D - b : 0) * ROWS + (b ? CHZ_HIST - 1 : CHZ_HIST) + lane;
		const float2 *gp = g + b;
		const int na = b ? CHZ_HIST : CHZ_HIST + 1;
		for (int i = 0; i < na; ++i) {
			const float2 t = gp[i * D];
			#pragma unroll
			for (int r = 0; r < R; ++r)
				K::mac(re[r], im[r], t.x, t.y, xp[64 * r - i]);
		}
	}
	float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
	#pragma unroll
	for (int r = 0; r < R; ++r) {
		const long long j = (long long)blockIdx.x * TILE + lane + 64 * r;   // the output's place in its row
		if (j >= a.n_out)
			continue;
		dst[j] = rotated<REAL>(re[r], im[r], inc * (unsigned)(unsigned long long)((a.out_first + j) * D));
	}
}

// what a workgroup's tile of k_rechannelize looks like: T, the outputs per residue M (a tile is q M outputs), the rows of history,
// the rows of a plane in LDS, the slots per lane (64 passes >= q M), the dynamic LDS in bytes
struct RechannelizeShape { int n_taps, m, hist, rows, passes; size_t lds; };

template <bool REAL, int FMT, int NP>
__global__ __launch_bounds__(64 * CHZ_WAVES) void k_rechannelize(ChannelizeArgs a, RechannelizeShape g)
{
	using K = Capture<REAL>;
	using X = typename K::sample;
	extern __shared__ float2 rcz_lds[];
	const int P = a.p, Q = a.q, T = g.n_taps, M = g.m, H = g.hist, ROWS = g.rows;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	X *xs = K::span_first ? (X *)rcz_lds : (X *)(rcz_lds + CHZ_WAVES * T);            // [P][ROWS]
	float2 *ph = (K::span_first ? rcz_lds + P * ROWS : rcz_lds) + w * T;              // [CHZ_WAVES][T]
	const int tile = Q * M;
	const long long t = a.out_first / tile + (long long)blockIdx.x;   // the tile, counted from output 0
	const long long m_lo = (t * M - H) * P;                       // i_n of the tile's first output is t M P
	const int span = (M + H) * P;
	for (int s = tid; s < span; s += 64 * CHZ_WAVES) {
		const long long m = m_lo + s;
		X v = K::zero();
		if (m >= a.in_first && m - a.in_first < a.n_in)
			v = K::template load<FMT>(a.in, (size_t)(m - a.in_first));
		const int row = s / P, pl = s - row * P;
		xs[pl * ROWS + row] = v;
	}
	const int c = (int)blockIdx.y * CHZ_WAVES + w;
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
			const X x = xs[at[r]];                                        // (spelt out: profiles/channelize_one_kernel.txt)
			K::mac(re[r], im[r], gx, gy, x);
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
		dst[j] = rotated<REAL>(re[r], im[r], inc * (unsigned)i_n);
	}
}

// ---- the shapes.  span_bytes: 8 for an analytic capture's span, 4 for a real one's
constexpr size_t span_bytes(bool real) { return real ? sizeof(float) : sizeof(float2); }

// k_channelize's outputs per lane, from the LDS budget: a tile of 64 R outputs costs 8 x 4 (24 D + 1) bytes of modulated taps and
// span_bytes x D (64 R + 25) of span.  An analytic capture has R = 4 up to D = 16 (3784 D + 32 bytes: 48288 there) and R = 2 above
// (63776 at D = 32); a real one has ONE shape, R = 4 at 1892 D + 32 bytes - 60576 at D = 32.  (R = 8 would fit a real capture up to
// D = 22 only and is not taken: it halves the workgroups of a bank's push, which has few, and would bring a change of shape back.)
constexpr int channelize_outputs_per_lane(int d, bool real) { return real || d <= 16 ? CHZ_SLOTS : 2; }
constexpr size_t channelize_lds(int d, int r, bool real)
{
	return (size_t)CHZ_WAVES * (size_t)(24 * d + 1) * sizeof(float2) + (size_t)d * (size_t)(64 * r + CHZ_HIST + 1) * span_bytes(real);
}
static_assert(channelize_lds(16, channelize_outputs_per_lane(16, false), false) == 48288, "the byte counts above");
static_assert(channelize_lds(32, channelize_outputs_per_lane(32, false), false) == 63776 && 63776 <= CHZ_LDS, "D = 32 must fit");
static_assert(channelize_lds(32, channelize_outputs_per_lane(32, true), true) == 60576 && 60576 <= CHZ_LDS, "D = 32 must fit");

// k_rechannelize's M outputs per residue and tile: as many as leave the span [P][(M + H) | 1] and the four waves' phasors inside
// CHZ_LDS (for an analytic capture the fewest are 7, at 511/16: 9 rows of 511 samples and 4 x 767 phasors are 61336 bytes; a real
// one has twice the rows and 17 there), and at most 64 NP / Q for NP slots per lane; NP is the largest of 4 .. 1 at which 85 % of
// the 64 NP slots hold an output (NP = 1 fills them all but for Q M < 64)
constexpr RechannelizeShape rechannelize_shape(int p, int q, bool real)
{
	RechannelizeShape g{};
	g.n_taps = 24 * p / q + 1;
	g.hist = (g.n_taps - 1 + p - 1) / p;
	int rows = (int)((CHZ_LDS - (size_t)CHZ_WAVES * (size_t)g.n_taps * sizeof(float2)) / span_bytes(real) / (size_t)p);
	if (rows % 2 == 0)
		rows -= 1;
	const int m_lds = rows - g.hist;
	for (g.passes = CHZ_SLOTS; g.passes >= 1; --g.passes) {
		g.m = 64 * g.passes / q < m_lds ? 64 * g.passes / q : m_lds;
		if (100 * q * g.m >= 85 * 64 * g.passes || g.passes == 1)
			break;
	}
	g.rows = (g.m + g.hist) | 1;
	g.lds = (size_t)p * (size_t)g.rows * span_bytes(real) + (size_t)CHZ_WAVES * (size_t)g.n_taps * sizeof(float2);
	return g;
}

// every admitted ratio (gcd(p, q) = 1, 2 <= q <= 16, 2 q <= p <= 32 q): both kinds fit the LDS, no tile is shorter than the 32
// outputs channelize_max_outputs counts on, and a real capture's rows never bind - it always has 4 slots per lane, so that
// k_rechannelize<true, ., NP> exists at NP = 4 only
constexpr bool rechannelize_shapes_hold()
{
	for (int q = 2; q <= 16; ++q)
		for (int p = 2 * q; p <= 32 * q; ++p) {
			int a = p, b = q;
			while (b) {
				const int r = a % b;
				a = b;
				b = r;
			}
			if (a != 1)
				continue;
			const RechannelizeShape z = rechannelize_shape(p, q, false), x = rechannelize_shape(p, q, true);
			if (z.lds > CHZ_LDS || x.lds > CHZ_LDS || q * z.m < 32 || x.m < z.m || x.passes != CHZ_SLOTS)
				return false;
		}
	return true;
}
static_assert(rechannelize_shapes_hold(), "a real capture must get 4 slots per lane at every admitted ratio");

// (the shortest tile is 128 outputs at q = 1 and no shorter than 32 otherwise, for either kind of capture - a real one's tiles are
// no shorter than an analytic one's: the grid's x stays below 2^31)
long long channelize_max_outputs(int q) { return (q == 1 ? 128LL : 32LL) * 0x7fffffffLL; }

// ---- the dispatch: the kind of capture and the format here, R or NP from the shape
template <bool REAL, int FMT, int R> static void chz_launch(hipStream_t s, const ChannelizeArgs &a)
{
	const unsigned groups = (unsigned)((a.n_channels + CHZ_WAVES - 1) / CHZ_WAVES);
	hipLaunchKernelGGL((k_channelize<REAL, FMT, R>), dim3((unsigned)((a.n_out + 64 * R - 1) / (64 * R)), groups), dim3(64 * CHZ_WAVES), channelize_lds(a.p, R, REAL), s, a);
}

template <bool REAL, int FMT, int NP> static void rcz_launch(hipStream_t s, const ChannelizeArgs &a, const RechannelizeShape &g)
{
	const long long tile = (long long)a.q * g.m;
	const long long tiles = (a.out_first + a.n_out - 1) / tile - a.out_first / tile + 1;
	const unsigned groups = (unsigned)((a.n_channels + CHZ_WAVES - 1) / CHZ_WAVES);
	hipLaunchKernelGGL((k_rechannelize<REAL, FMT, NP>), dim3((unsigned)tiles, groups), dim3(64 * CHZ_WAVES), g.lds, s, a, g);
}

template <bool REAL, int FMT> static void launch_kind(hipStream_t s, const ChannelizeArgs &a)
{
	// (a real capture always has 4 per lane: channelize_outputs_per_lane, and the static_assert over the ratios)
	if (a.q == 1) {
		if (channelize_outputs_per_lane(a.p, REAL) == 4)
			chz_launch<REAL, FMT, 4>(s, a);
		else if constexpr (!REAL)
			chz_launch<REAL, FMT, 2>(s, a);
		return;
	}
	const RechannelizeShape g = rechannelize_shape(a.p, a.q, REAL);
	if (g.passes == 4)
		rcz_launch<REAL, FMT, 4>(s, a, g);
	else if constexpr (!REAL) {
		if (g.passes == 3)
			rcz_launch<REAL, FMT, 3>(s, a, g);
		else if (g.passes == 2)
			rcz_launch<REAL, FMT, 2>(s, a, g);
		else
			rcz_launch<REAL, FMT, 1>(s, a, g);
	}
}

void launch_channelize(hipStream_t s, const ChannelizeArgs &a)
{
	switch ((a.real ? 3 : 0) + a.fmt) {
	case 0: return launch_kind<false, 0>(s, a);
	case 1: return launch_kind<false, 1>(s, a);
	case 2: return launch_kind<false, 2>(s, a);
	case 3: return launch_kind<true, 0>(s, a);
	case 4: return launch_kind<true, 1>(s, a);
	default: return launch_kind<true, 2>(s, a);
	}
}

}  // namespace rx
