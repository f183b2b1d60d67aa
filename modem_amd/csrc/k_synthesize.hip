// k_synthesize.hip -- the wideband synthesizer, the mirror image of k_channelize.hip: n_channels narrowband
// transmissions at the handle's rate -> one wideband I/Q capture at D x that rate.  Each channel is zero-stuffed by D, low-pass
// filtered with the channelizer's own 24 D + 1 taps, mixed up to its centre by the integer-phase NCO of 4.14 and added in at its
// start and gain.  Every output is a closed form of absolute sample indices, so the kernel has no state and a capture cuts into
// windows without changing a bit.  At absolute wideband index m, with r = m - start_c, q = floor(r / D), b = r - q D:
//   u_c[m] = sum_a h[b + a D] x_c[q - a],  a = 0 .. 23, and a = 24 where b = 0;  x_c zero outside 0 .. n_in - 1
//   w[m]   = sum_c G_c e^{+2 pi i phi_c(m) / 2^32} u_c[m],                        phi_c(m) = inc_c m mod 2^32
// One workgroup of 256 threads makes a tile of (256 / D) D SYN_R outputs.  Thread t = g D + t' (g < 256 / D; the few threads behind
// are idle in the sum) makes the SYN_R outputs (g SYN_R + i) D + t', i = 0 .. SYN_R - 1, of the tile: they are D apart, so for any
// channel they share b - and with it the 24 (25) taps h[b + a D], read once into registers - and meet consecutive inputs, a window
// of SYN_R + 24 sample frames read once: 53 LDS reads for 5 x 48 multiply-adds.  The workgroup walks the channels in ascending
// order and skips, with a workgroup-uniform branch, every channel whose support [start_c, start_c + (n_in - 1) D + 24 D] misses the
// tile.  For a channel that meets it, the tile's span of input - tile / D + 25 sample frames - is converted once to fp32 and laid
// in LDS; the next such channel's span is loaded into registers before the current one is summed and goes into the other half of
// a double buffer after it, so the loads are in flight during the sum and one barrier per channel suffices.  Lanes of one g read
// neighbouring taps and broadcast their inputs; lanes of neighbouring g read inputs SYN_R float2 apart, and SYN_R is odd, so that
// the 32 lanes of a half wave fall on different bank pairs (a carry of one sample between the lanes of a g can cost a 2-way conflict).
// The order is part of the definition's contract and a function of (c, m) alone: u_c is one chain of fused multiply-adds per
// component with a ascending from +0; (cs, sn) = sincospif of the phase as a signed fraction of a turn (phase_phasor, dev_common.h);
// gr = G_c cs, gi = G_c sn; then re: + gr u.re, - gi u.im; im: + gr u.im, + gi u.re, one chain per component over c ascending from
// +0.  A term whose input lies outside 0 .. n_in - 1 multiplies +0 and a channel that misses the tile adds +0 four times: neither
// changes a value.  It can change the sign of a zero - a product that underflows to -0 stays -0 only until a +0 is added - so every
// output passes through v + 0.f before it is stored: a zero is always written as +0, and skipping changes no byte.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int SYN_THREADS = 256;
constexpr int SYN_R = 5;                                          // outputs per thread, D apart; odd (see above)
constexpr int SYN_HIST = 24;                                      // (T - 1) / D
constexpr int SYN_WIN = SYN_R + SYN_HIST;                         // inputs a thread's outputs meet
constexpr int SYN_SPAN = (SYN_THREADS / 2) * SYN_R + SYN_HIST + 2;   // input sample frames a tile can meet, at D = 2 (and one spare)
constexpr int SYN_PRE = (SYN_SPAN + SYN_THREADS - 1) / SYN_THREADS;
constexpr int SYN_TAPS = 24 * 32 + 1;

__host__ __device__ inline int syn_tile(int D) { return (SYN_THREADS / D) * D * SYN_R; }

// IFMT: 0 S16, 2 F32 input; OFMT: 0 S16, 2 F32 output
template <int IFMT, int OFMT>
__global__ __launch_bounds__(SYN_THREADS) void k_synthesize(SynthesizeArgs a)
{
	__shared__ float hs[SYN_TAPS];
	__shared__ float2 xs[2][SYN_SPAN];
	const int D = a.p, T = 2 * 12 * D + 1;
	const int G = SYN_THREADS / D, TILE = G * D * SYN_R;
	const int tid = threadIdx.x;
	const int g = tid / D, tp = tid - g * D;
	const bool active = g < G;
	const long long t0 = (long long)blockIdx.x * TILE;                // the tile's place in the window
	const long long m0 = a.out_first + t0;
	const long long left = a.n_out - t0;
	const int n_tile = left < TILE ? (int)left : TILE;
	const long long m_hi = m0 + n_tile - 1;
	const long long reach = (a.n_in - 1) * D + (T - 1);               // a channel's support is start .. start + reach
	const int span = G * SYN_R + SYN_HIST + 1;                        // <= SYN_SPAN - 1
	for (int k = tid; k < T; k += SYN_THREADS)
		hs[k] = a.taps[k];
	float wr[SYN_R], wi[SYN_R];
	#pragma unroll
	for (int i = 0; i < SYN_R; ++i)
		wr[i] = wi[i] = 0.f;
	// the next channel at or after c that meets the tile (n_channels: none) - the same for every thread
	auto next_hit = [&](int c) {
		for (; c < a.n_channels; ++c) {
			const long long s = a.ch[c].start;
			if (s <= m_hi && s + reach >= m0)
				break;
		}
		return c;
	};
	// input sample frame j_lo + s of channel c for s = tid, tid + 256, ..: zeros outside 0 .. n_in - 1, which are never loaded
	float2 pre[SYN_PRE];
	auto fetch = [&](int c) {
		const long long j_lo = floor_div(m0 - a.ch[c].start - (T - 1), D);
		const size_t row = (size_t)c * (size_t)a.in_stride;
		#pragma unroll
		for (int p = 0; p < SYN_PRE; ++p) {
			const int s = tid + SYN_THREADS * p;
			const long long j = j_lo + s;
			pre[p] = make_float2(0.f, 0.f);
			if (s < span && j >= 0 && j < a.n_in)
				pre[p] = iq_sample<IFMT>(a.in, row + (size_t)j);
		}
	};
	auto stash = [&](int buf) {
		#pragma unroll
		for (int p = 0; p < SYN_PRE; ++p) {
			const int s = tid + SYN_THREADS * p;
			if (s < span)
				xs[buf][s] = pre[p];
		}
	};
	int c = next_hit(0), cur = 0;
	if (c < a.n_channels) {
		fetch(c);
		stash(0);
	}
	__syncthreads();
	while (c < a.n_channels) {
		const int cn = next_hit(c + 1);
		if (cn < a.n_channels)
			fetch(cn);
		if (active) {
			const SynthChannel ch = a.ch[c];
			const long long r_lo = m0 - ch.start - (T - 1);
			const int e = (int)(r_lo - floor_div(r_lo, D) * D);       // 0 .. D - 1: output t of the tile has r = (24 + j_lo) D + e + t
			int b = tp + e, s0 = g * SYN_R;                            // output i: b, and q - j_lo = 24 + s0 + i
			if (b >= D) {
				b -= D;
				++s0;
			}
			float hb[SYN_HIST];
			#pragma unroll
			for (int k = 0; k < SYN_HIST; ++k)
				hb[k] = hs[b + k * D];
			const float h24 = hs[SYN_HIST * D];                        // the 25th term's tap, where b = 0
			float2 xw[SYN_WIN];                                        // s0 + SYN_WIN - 1 <= (G - 1) SYN_R + 1 + SYN_R + 23 = span - 1
			#pragma unroll
			for (int k = 0; k < SYN_WIN; ++k)
				xw[k] = xs[cur][s0 + k];
			#pragma unroll
			for (int i = 0; i < SYN_R; ++i) {
				float ur = 0.f, ui = 0.f;
				#pragma unroll
				for (int k = 0; k < SYN_HIST; ++k) {
					const float2 x = xw[SYN_HIST + i - k];
					ur = __builtin_fmaf(hb[k], x.x, ur);
					ui = __builtin_fmaf(hb[k], x.y, ui);
				}
				if (b == 0) {
					ur = __builtin_fmaf(h24, xw[i].x, ur);
					ui = __builtin_fmaf(h24, xw[i].y, ui);
				}
				float cs, sn;
				phase_phasor(ch.inc * (unsigned)(unsigned long long)(m0 + (g * SYN_R + i) * D + tp), cs, sn);
				const float gr = ch.gain * cs, gi = ch.gain * sn;
				wr[i] = __builtin_fmaf(gr, ur, wr[i]);
				wr[i] = __builtin_fmaf(-gi, ui, wr[i]);
				wi[i] = __builtin_fmaf(gr, ui, wi[i]);
				wi[i] = __builtin_fmaf(gi, ur, wi[i]);
			}
		}
		if (cn < a.n_channels)
			stash(cur ^ 1);
		__syncthreads();
		c = cn;
		cur ^= 1;
	}
	if (!active)
		return;
	#pragma unroll
	for (int i = 0; i < SYN_R; ++i) {
		const int t = (g * SYN_R + i) * D + tp;
		if (t >= n_tile)
			continue;
		iq_store<OFMT>(a.out, t0, t, wr[i], wi[i]);                       // (-0 -> +0: see the header)
	}
}

// (k_synthesize's smallest tile is 1160 outputs, at D = 29; k_resynthesize's is 1024: the grid's x stays below 2^31)
long long synthesize_max_outputs(int) { return 1024LL * 0x7fffffffLL; }

void launch_synthesize(hipStream_t s, const SynthesizeArgs &a)
{
	if (a.q != 1)
		return launch_synthesize_ratio(s, a);
	const int tile = syn_tile(a.p);
	const dim3 grid((unsigned)((a.n_out + tile - 1) / tile)), block(SYN_THREADS);
	if (a.in_fmt == 0 && a.out_fmt == 0)
		hipLaunchKernelGGL((k_synthesize<0, 0>), grid, block, 0, s, a);
	else if (a.in_fmt == 0)
		hipLaunchKernelGGL((k_synthesize<0, 2>), grid, block, 0, s, a);
	else if (a.out_fmt == 0)
		hipLaunchKernelGGL((k_synthesize<2, 0>), grid, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_synthesize<2, 2>), grid, block, 0, s, a);
}

}  // namespace rx
