// k_resynthesize.hip -- the wideband synthesizer at a rational interpolation P / Q, the mirror image of
// k_rechannelize (k_channelize.hip): n_channels narrowband transmissions at the handle's rate -> one wideband I/Q capture at rate P / Q.  Like
// k_synthesize every output is a closed form of absolute sample indices, so the kernel has no state and a capture cuts into windows
// without changing a bit.  G[tn], tn = 0 .. 24 P, is the ratio front end's fp32 tap table read as one sequence on the grid of 1 / Q
// wideband samples (G[tn] = H[tn mod Q][tn div Q]).  At absolute wideband index m, with r = m - start_c, nu = r Q, q0 = nu div P,
// b = nu mod P:
//   u_c[m] = sum_a G[b + a P] x_c[q0 - a],  a = 0 .. 23, and a = 24 where b = 0;  x_c zero outside 0 .. n_in - 1
//   w[m]   = sum_c G_c e^{+2 pi i phi_c(m) / 2^32} u_c[m],                         phi_c(m) = inc_c m mod 2^32
// One workgroup of 256 threads makes a tile of 256 RSY_R consecutive outputs; thread t makes the outputs t, t + 256, .. of the tile.
// The taps lie in device memory transposed, [P][RSY_ROW]: row b holds G[b + a P], a = 0 .. 24 (zeros where b + a P > 24 P), so that
// an output reads its 25 taps with seven 16-byte loads; the table is at most 511 rows of 112 bytes and stays in the caches.  The
// workgroup walks the channels in ascending order and skips, with a workgroup-uniform branch, every channel whose support
// [start_c, start_c + (n_in + 23) P div Q] misses the tile.  For a channel that meets it, the tile's span of input - at most
// tile Q / P + 26 sample frames - is converted once to fp32 and laid in LDS; the next such channel's span is loaded into registers
// before the current one is summed and goes into the other half of a double buffer after it, so the loads are in flight during the
// sum and one barrier per channel suffices.  Neighbouring lanes meet the same input or the next (Q / P <= 1 / 2): their LDS reads
// are broadcasts or fall on neighbouring banks.
// Index arithmetic: the tile's first output has nu0 = (m0 - start_c) Q = qb P + bb, one 64-bit floored division that is the same
// for every thread; thread t's first output then needs one 32-bit division, (bb + t Q) / P, and its later outputs step by the
// quotient and remainder of 256 Q / P.  Nothing is divided inside the tap loop.
// The order is part of the definition's contract and a function of (c, m) alone, as in k_synthesize: u_c is one chain of fused
// multiply-adds per component with a ascending from +0, the 25th term taken under a predicate where b = 0 (never multiplied by a
// zero tap: F32 input may hold non-finite values); (cs, sn) = sincospif of the phase as a signed fraction of a turn; gr = G_c cs,
// gi = G_c sn; then re: + gr u.re, - gi u.im; im: + gr u.im, + gi u.re, one chain per component over c ascending from +0.  An
// input outside 0 .. n_in - 1 enters as +0 and a channel that misses the tile adds nothing; every output passes through v + 0.f
// before it is stored, so a zero is always written as +0 and skipping changes no byte.
#include "dev_common.h"
#include "kernels.h"

namespace rx {

constexpr int RSY_THREADS = 256;
constexpr int RSY_R = 4;                                          // outputs per thread, 256 apart
constexpr int RSY_TILE = RSY_THREADS * RSY_R;
constexpr int RSY_HIST = 24;
// input sample frames a tile can meet: the first output's q0 - 24 .. the last output's q0, and q0 grows over the tile by at most
// (P - 1 + (RSY_TILE - 1) Q) div P <= (RSY_TILE - 1) / 2 + 1 (Q / P <= 1 / 2)
constexpr int RSY_SPAN = RSY_HIST + (RSY_TILE - 1) / 2 + 1 + 1;
constexpr int RSY_PRE = (RSY_SPAN + RSY_THREADS - 1) / RSY_THREADS;

// IFMT: 0 S16, 2 F32 input; OFMT: 0 S16, 2 F32 output.  The second launch bound holds the kernel to 128 VGPRs, four waves per SIMD
// (it takes 130 - 132 and three without it, and the end-to-end case is 17 % slower: profiles/resynthesize.txt)
template <int IFMT, int OFMT>
__global__ __launch_bounds__(RSY_THREADS, 4) void k_resynthesize(SynthesizeArgs a)
{
	__shared__ float2 xs[2][RSY_SPAN];
	const int P = a.p, Q = a.q;
	const int tid = threadIdx.x;
	const long long t0 = (long long)blockIdx.x * RSY_TILE;            // the tile's place in the window
	const long long m0 = a.out_first + t0;
	const long long left = a.n_out - t0;
	const int n_tile = left < RSY_TILE ? (int)left : RSY_TILE;
	const long long m_hi = m0 + n_tile - 1;
	const long long reach = ((a.n_in - 1 + RSY_HIST) * P) / Q;        // a channel's support is start .. start + reach
	const int span = RSY_HIST + (P - 1 + (RSY_TILE - 1) * Q) / P + 1;   // <= RSY_SPAN
	const int step_q = (RSY_THREADS * Q) / P, step_b = RSY_THREADS * Q - step_q * P;   // 256 outputs on: q0 + step_q, b + step_b
	float wr[RSY_R], wi[RSY_R];
	#pragma unroll
	for (int i = 0; i < RSY_R; ++i)
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
	float2 pre[RSY_PRE];
	auto fetch = [&](int c) {
		const long long j_lo = floor_div((m0 - a.ch[c].start) * Q, P) - RSY_HIST;
		const size_t row = (size_t)c * (size_t)a.in_stride;
		#pragma unroll
		for (int p = 0; p < RSY_PRE; ++p) {
			const int s = tid + RSY_THREADS * p;
			const long long j = j_lo + s;
			pre[p] = make_float2(0.f, 0.f);
			if (s < span && j >= 0 && j < a.n_in)
				pre[p] = iq_sample<IFMT>(a.in, row + (size_t)j);
		}
	};
	auto stash = [&](int buf) {
		#pragma unroll
		for (int p = 0; p < RSY_PRE; ++p) {
			const int s = tid + RSY_THREADS * p;
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
		const SynthChannel ch = a.ch[c];
		const long long nu0 = (m0 - ch.start) * Q;
		const int bb = (int)(nu0 - floor_div(nu0, P) * P);            // 0 .. P - 1: output t of the tile has nu = (j_lo + 24) P + bb + t Q
		const unsigned tq = (unsigned)(bb + tid * Q);                 // < 512 + 255 x 16
		int s = (int)(tq / (unsigned)P), b = (int)tq - s * P;         // output i: b, and q0 - j_lo = 24 + s
		#pragma unroll
		for (int i = 0; i < RSY_R; ++i) {
			// s + 24 <= 24 + (P - 1 + (RSY_TILE - 1) Q) div P = span - 1
			const float4 *row = (const float4 *)(a.taps + (size_t)b * RSY_ROW);
			float h[RSY_ROW];
			#pragma unroll
			for (int k = 0; k < RSY_ROW / 4; ++k) {
				const float4 v = row[k];
				h[4 * k] = v.x;
				h[4 * k + 1] = v.y;
				h[4 * k + 2] = v.z;
				h[4 * k + 3] = v.w;
			}
			const float2 *x = &xs[cur][s + RSY_HIST];
			float ur = 0.f, ui = 0.f;
			#pragma unroll
			for (int k = 0; k < RSY_HIST; ++k) {
				const float2 v = x[-k];
				ur = __builtin_fmaf(h[k], v.x, ur);
				ui = __builtin_fmaf(h[k], v.y, ui);
			}
			if (b == 0) {
				const float2 v = x[-RSY_HIST];
				ur = __builtin_fmaf(h[RSY_HIST], v.x, ur);
				ui = __builtin_fmaf(h[RSY_HIST], v.y, ui);
			}
			float cs, sn;
			phase_phasor(ch.inc * (unsigned)(unsigned long long)(m0 + tid + RSY_THREADS * i), cs, sn);
			const float gr = ch.gain * cs, gi = ch.gain * sn;
			wr[i] = __builtin_fmaf(gr, ur, wr[i]);
			wr[i] = __builtin_fmaf(-gi, ui, wr[i]);
			wi[i] = __builtin_fmaf(gr, ui, wi[i]);
			wi[i] = __builtin_fmaf(gi, ur, wi[i]);
			s += step_q;
			b += step_b;
			if (b >= P) {
				b -= P;
				++s;
			}
		}
		if (cn < a.n_channels)
			stash(cur ^ 1);
		__syncthreads();
		c = cn;
		cur ^= 1;
	}
	#pragma unroll
	for (int i = 0; i < RSY_R; ++i) {
		const int t = tid + RSY_THREADS * i;
		if (t >= n_tile)
			continue;
		iq_store<OFMT>(a.out, t0, t, wr[i], wi[i]);                       // (-0 -> +0: see the header)
	}
}

static_assert(RSY_TILE == 1024, "synthesize_max_outputs (k_synthesize.hip) counts on tiles of 1024 outputs");

void launch_synthesize_ratio(hipStream_t s, const SynthesizeArgs &a)
{
	const dim3 grid((unsigned)((a.n_out + RSY_TILE - 1) / RSY_TILE)), block(RSY_THREADS);
	if (a.in_fmt == 0 && a.out_fmt == 0)
		hipLaunchKernelGGL((k_resynthesize<0, 0>), grid, block, 0, s, a);
	else if (a.in_fmt == 0)
		hipLaunchKernelGGL((k_resynthesize<0, 2>), grid, block, 0, s, a);
	else if (a.out_fmt == 0)
		hipLaunchKernelGGL((k_resynthesize<2, 0>), grid, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_resynthesize<2, 2>), grid, block, 0, s, a);
}

}  // namespace rx
