// k_synthesize_grid_ratio.hip -- the wideband synthesizer on a channel grid at any ratio P / Q, the mirror
// image of k_channelize_grid_ratio.hip: section 4.20's polyphase synthesis bank with section 4.18's taps and output times and section
// 4.22's mixed-radix transform, run the other way.  P / Q in lowest terms, 1 <= Q <= 16, 2 Q <= P <= 512, P = 2^a 3^b 5^c (not Q = 1
// with P a power of two: that is 4.20's kernels); M = 2 P; G[tn], tn = 0 .. 24 P, section 4.18's tap sequence.  Row c belongs to slot
// k_c (-P <= k_c Q < P, pairwise distinct) at k_c Q / M cycles per wideband sample, starts at the wideband index sigma_c P - Q sigma_c
// input samples in - and has the gain G_c = (P / Q) gain_c.  At the absolute wideband index m, m Q = J P + beta (0 <= beta < P):
//   w[m] = sum_c G_c e^{+2 pi i (k_c Q m mod M) / M} sum_a G[beta + a P] x_c[J - a - sigma_c Q],   a = 0 .. 23, and a = 24 where beta = 0,
// computed as
//   X_j[(-k_c) mod M] = (-1)^{k_c j} (G_c x_c[j - sigma_c Q]),  every other entry +0                 (j: absolute input time)
//   V_j[r] = sum_b X_j[b] e^{-2 pi i b r / M},  r = 0 .. M - 1                                        (the FORWARD transform)
//   w[m]   = sum_a G[beta + a P] V_{J - a}[beta + (a mod 2) P];  V_j = 0 for j < 0.
// (k Q m / M = k j / 2 + k (beta + a P) / M with j = J - a: the first term is the sign; the slot at bin -k turns the inverse sum into
// the forward one, which dev_common.h's Bfly<2 / 3 / 4 / 5> compute.)  Two kernels, with V in the scratch as [time][r], r natural:
//   k_synthesize_grid_ratio_transform: one workgroup of 256 threads makes a tile of NT input times in dynamic LDS, u[row][t] (time
//     minor, rows of NT + 1).  It clears the tile, places the rows' samples - lanes along time - at the row where
//     channelize_grid_ratio_row puts bin (-k) mod M, and runs the transform in place, decimation in time: section 4.22's stages in
//     reverse order (a lone 2, the 4s, the 3s, the 5s).  A stage of radix R on blocks of N = R L points: the points i + t L,
//     t = 1 .. R - 1 (j = i mod L), are multiplied by w^{j t M / N}, w = e^{-2 pi i / M} (not at L = 1, where the root is 1), then go
//     through Bfly<R> and back in place: the transposed flow graph of k_channelize_grid_ratio.hip's cgr_stage.  Digit-reversed order
//     in, natural order out.  The order of every sum is fixed by M alone.  A tile no row reaches writes +0 and skips the rest
//     (workgroup-uniform).
//   k_synthesize_grid_ratio_filter: a lane per output m, a tile of 256 SGR_R consecutive outputs per workgroup, thread t the outputs
//     t, t + 256 ...  k_resynthesize's index arithmetic: one 64-bit division per workgroup for the tile's first m Q, one 32-bit
//     division per lane for (J, beta), steps by the quotient and remainder of 256 Q / P after that.  The lane's taps are row beta of
//     section 4.18's transposed table [P][RSY_ROW] (seven 16-byte loads); 25 loads of V, at rows beta and beta + P alternately.
//     Neighbouring lanes read V rows Q apart.  This is the form for Q > 1.
//   k_synthesize_grid_ratio_slide: the form for Q = 1, where beta = m mod P runs along the lanes: section 4.20's sliding form with a
//     run-time P.  Work item (g, beta) makes the SGR_S outputs (q0 + i) P + beta, i = 0 .. SGR_S - 1, P apart: they share their taps in
//     registers and slide over the two V rows beta and beta + P of SGR_S + 24 times, newest first, so that every output's chain still
//     runs with a ascending.  A tile is 256 / P groups (one from P = 256 on) of SGR_S output times, counted from the chunk's first.
// Contract on order: G_c x is one fp32 product per component; w is one FMA chain per component from +0, a ascending, the 25th term
// under a predicate (beta = 0), never through a zero tap; every output passes through v + 0.f (iq_store).  No state: V_j is a function
// of j alone, so windows, tiles and the host's chunks change no byte.
#include "dev_common.h"
#include "grid_bank.h"
#include "kernels.h"

namespace rx {

constexpr int SGR_THREADS = 256;
constexpr int SGR_HIST = 24;
constexpr int SGR_R = 4;                                          // outputs per thread of the filter, 256 apart
constexpr int SGR_TILE = SGR_THREADS * SGR_R;
constexpr int SGR_LDS = 61440;                                    // bytes of a transform tile at most

__device__ __forceinline__ cf sgr_mul(cf a, float2 w)
{
	const float2 v = grid_mul(make_float2(a.re, a.im), w);
	return mk(v.x, v.y);
}

// one decimation-in-time stage of radix R on blocks of N points, every time of the tile
template <int R> __device__ __forceinline__ void sgr_stage(cf *u, const float2 *tw, int tid, int M, int N, int NT)
{
	const int NTS = NT + 1, L = N / R, step = M / N, nb = M / R;
	for (int it = tid; it < nb * NT; it += SGR_THREADS) {
		int b, t;
		if (NT >= 32) {                                               // lanes along t where a tile has that many times
			b = it / NT;
			t = it - b * NT;
		} else {
			t = it / nb;
			b = it - t * nb;
		}
		const int blk = b / L, j = b - blk * L;
		cf *x = u + (blk * N + j) * NTS + t;
		cf v[R];
		#pragma unroll
		for (int i = 0; i < R; ++i)
			v[i] = x[i * L * NTS];
		if (L > 1) {
			#pragma unroll
			for (int i = 1; i < R; ++i)
				v[i] = sgr_mul(v[i], tw[j * i * step]);
		}
		Bfly<R>::run(v);
		#pragma unroll
		for (int i = 0; i < R; ++i)
			x[i * L * NTS] = v[i];
	}
	__syncthreads();
}

template <int IFMT>
__global__ __launch_bounds__(SGR_THREADS) void k_synthesize_grid_ratio_transform(SynthesizeGridRatioArgs a)
{
	extern __shared__ float2 sgr_lds[];
	const int M = a.m, NT = a.nt, NTS = NT + 1;
	cf *u = (cf *)sgr_lds;                                        // [M][NTS]
	const int tid = threadIdx.x;
	const int t0 = blockIdx.x * NT;                               // the tile's first time in the scratch
	const long long j0 = a.j_first + t0;                          // ... as an absolute input time (may be negative: V is zero there)
	float2 *dst = a.scratch + (size_t)t0 * (size_t)M;             // the tile's M NT points, [time][r]: index t M + r

	// does any row reach the tile?  Row c holds the times ch[c].start .. ch[c].start + n_in - 1
	int hit = 0;
	for (int c = tid; c < a.n_channels; c += SGR_THREADS) {
		const long long sg = a.ch[c].start;
		hit |= sg <= j0 + NT - 1 && sg + a.n_in - 1 >= j0;
	}
	if (!__syncthreads_or(hit)) {
		for (int it = tid; it < M * NT; it += SGR_THREADS)
			dst[it] = make_float2(0.f, 0.f);
		return;
	}

	// ---- 1. X: zeros, then the rows' samples at the row of bin (-k) mod M; (-1)^{k j}.  The slots are distinct: no two items share a point
	for (int it = tid; it < M * NTS; it += SGR_THREADS)
		u[it] = mk(0.f, 0.f);
	__syncthreads();
	for (int it = tid; it < a.n_channels * NT; it += SGR_THREADS) {
		const int c = it / NT, t = it - c * NT;
		const SynthChannel ch = a.ch[c];
		const long long j = j0 + t, i = j - ch.start;
		if (i < 0 || i >= a.n_in)
			continue;
		const float2 x = iq_sample<IFMT>(a.in, (size_t)c * (size_t)a.in_stride + (size_t)i);
		cf v = mk(ch.gain * x.x, ch.gain * x.y);
		if ((ch.inc >> 16) & (unsigned)j & 1u)                        // inc = the row | (k mod 2) << 16
			v = mk(-v.re, -v.im);
		u[(int)(ch.inc & 0xffffu) * NTS + t] = v;
	}
	__syncthreads();

	// ---- 2. the transform: the plan's radices (four bits each, the front end's first stage lowest) from the last to the first
	{
		int ns = 0;
		while (ns < 8 && ((a.radices >> (4 * ns)) & 15u))
			++ns;
		int N = 1;
		for (int s = ns - 1; s >= 0; --s) {
			const int R = (int)((a.radices >> (4 * s)) & 15u);
			N *= R;
			switch (R) {
			case 5: sgr_stage<5>(u, a.tw, tid, M, N, NT); break;
			case 3: sgr_stage<3>(u, a.tw, tid, M, N, NT); break;
			case 4: sgr_stage<4>(u, a.tw, tid, M, N, NT); break;
			default: sgr_stage<2>(u, a.tw, tid, M, N, NT); break;
			}
		}
	}

	// ---- 3. V to the scratch, one contiguous run: point t M + r is row r, time t of the tile
	for (int it = tid; it < M * NT; it += SGR_THREADS) {
		const int t = it / M, r = it - t * M;
		const cf v = u[r * NTS + t];
		dst[it] = make_float2(v.re, v.im);
	}
}

template <int OFMT>
__global__ __launch_bounds__(SGR_THREADS) void k_synthesize_grid_ratio_filter(SynthesizeGridRatioArgs a)
{
	const int P = a.p, Q = a.q, M = a.m;
	const int tid = threadIdx.x;
	const long long t0 = (long long)blockIdx.x * SGR_TILE;            // the tile's place among the chunk's outputs
	const long long m0 = a.m_first + t0;
	const long long left = a.n_m - t0;
	const int n_tile = left < SGR_TILE ? (int)left : SGR_TILE;
	const long long nu0 = m0 * Q, jb = nu0 / P;                       // (m0 >= 0) the tile's first output: m0 Q = jb P + bb
	const int bb = (int)(nu0 - jb * P);
	const int tb = (int)(jb - a.j_first);                             // jb's place in the scratch: >= 24
	const int step_q = (SGR_THREADS * Q) / P, step_b = SGR_THREADS * Q - step_q * P;   // 256 outputs on: J + step_q, beta + step_b
	const unsigned tq = (unsigned)(bb + tid * Q);                     // < 512 + 255 x 16
	int s = (int)(tq / (unsigned)P), b = (int)tq - s * P;             // output i: beta = b, J = jb + s
	#pragma unroll
	for (int i = 0; i < SGR_R; ++i) {
		const int t = tid + SGR_THREADS * i;
		if (t < n_tile) {
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
			// time J of the scratch, rows beta and beta + P; the host lays the chunk's J - 24 .. J inside the scratch
			const float2 *v = a.scratch + (size_t)(tb + s) * (size_t)M + b;
			float wr = 0.f, wi = 0.f;
			#pragma unroll
			for (int k = 0; k < SGR_HIST; ++k) {
				const float2 x = v[-(ptrdiff_t)k * M + ((k & 1) ? P : 0)];
				wr = __builtin_fmaf(h[k], x.x, wr);
				wi = __builtin_fmaf(h[k], x.y, wi);
			}
			if (b == 0) {                                                 // tap a = 24 exists for beta = 0 alone
				const float2 x = v[-(ptrdiff_t)SGR_HIST * M];
				wr = __builtin_fmaf(h[SGR_HIST], x.x, wr);
				wi = __builtin_fmaf(h[SGR_HIST], x.y, wi);
			}
			iq_store<OFMT>(a.out, m0 - a.out_first, t, wr, wi);           // (-0 -> +0: see k_synthesize.hip's header)
		}
		s += step_q;
		b += step_b;
		if (b >= P) {
			b -= P;
			++s;
		}
	}
}

constexpr int SGR_S = 8;                                          // outputs per work item of the sliding form, P apart

template <int OFMT>
__global__ __launch_bounds__(SGR_THREADS) void k_synthesize_grid_ratio_slide(SynthesizeGridRatioArgs a)
{
	constexpr int R = SGR_S;
	const int P = a.p, M = a.m;
	const int G = P < SGR_THREADS ? SGR_THREADS / P : 1;              // groups of a tile
	const long long out_hi = a.m_first + a.n_m;
	const long long q_first = a.m_first / P;                          // the chunk's first output time: a.j_first + 24
	const int nq = (int)((out_hi - 1) / P - q_first + 1);
	for (int item = threadIdx.x; item < G * P; item += SGR_THREADS) {
		const int g = item / P, b = item - g * P;
		const int qs = (blockIdx.x * G + g) * R;                      // the item's first output time, counted from the chunk's first
		if (qs >= nq)
			continue;
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
		float wr[R], wi[R];
		#pragma unroll
		for (int i = 0; i < R; ++i)
			wr[i] = wi[i] = 0.f;
		// scratch time of absolute time j: j - (q_first - 24); the item's newest time is qs + R - 1 + 24 there (the host lays the
		// chunk's times, rounded up to R, inside the scratch)
		const float2 *v = a.scratch + (size_t)(qs + R - 1 + SGR_HIST) * (size_t)M + b;
		#pragma unroll
		for (int jj = 0; jj < R + SGR_HIST; ++jj) {                   // time q0 + R - 1 - jj: output i meets it at tap a = jj - (R - 1 - i)
			const float2 ve = v[-(ptrdiff_t)jj * M], vo = v[-(ptrdiff_t)jj * M + P];
			#pragma unroll
			for (int i = 0; i < R; ++i) {
				const int t = jj - (R - 1 - i);
				if (t < 0 || t > SGR_HIST)
					continue;
				const float2 x = (t & 1) ? vo : ve;
				if (t < SGR_HIST) {
					wr[i] = __builtin_fmaf(h[t], x.x, wr[i]);
					wi[i] = __builtin_fmaf(h[t], x.y, wi[i]);
				} else {                                                  // tap a = 24 exists for beta = 0 alone
					wr[i] = b == 0 ? __builtin_fmaf(h[t], x.x, wr[i]) : wr[i];
					wi[i] = b == 0 ? __builtin_fmaf(h[t], x.y, wi[i]) : wi[i];
				}
			}
		}
		#pragma unroll
		for (int i = 0; i < R; ++i) {
			const long long m = (q_first + qs + i) * P + b;
			if (qs + i >= nq || m < a.m_first || m >= out_hi)
				continue;
			iq_store<OFMT>(a.out, m - a.out_first, 0, wr[i], wi[i]);     // (-0 -> +0: see k_synthesize.hip's header)
		}
	}
}

// the tile of the transform kernel: the front end's plan gives M, the radices and the times per tile (4096 points, 8 .. 256 times
// where LDS allows it, an even number: rows of NT + 1 are an odd stride in LDS)
static void sgr_plan(SynthesizeGridRatioArgs &a)
{
	const GridRatioPlan pl = channelize_grid_ratio_plan(a.p, a.q);
	a.m = pl.m;
	a.nt = pl.nt;
	a.radices = pl.radices;
}

int synthesize_grid_ratio_tile_times(int p, int q) { return channelize_grid_ratio_plan(p, q).nt; }
// outputs per workgroup of the filter: Q > 1, counted from the chunk's first output; Q = 1, from its first output time
int synthesize_grid_ratio_filter_outputs(int p, int q) { return q > 1 ? SGR_TILE : (p < SGR_THREADS ? SGR_THREADS / p : 1) * SGR_S * p; }
int synthesize_grid_ratio_filter_round(int q) { return q > 1 ? 1 : SGR_S; }

void launch_synthesize_grid_ratio(hipStream_t s, const SynthesizeGridRatioArgs &args)
{
	SynthesizeGridRatioArgs a = args;
	sgr_plan(a);
	const size_t lds = (size_t)a.m * (size_t)(a.nt + 1) * sizeof(float2);   // <= SGR_LDS: the plan keeps 8 M (NT + 1) + 4 NT inside 60 KiB
	const dim3 tg((unsigned)(a.n_times / a.nt)), fg((unsigned)((a.n_m + SGR_TILE - 1) / SGR_TILE)), block(SGR_THREADS);
	if (a.in_fmt == 0)
		hipLaunchKernelGGL((k_synthesize_grid_ratio_transform<0>), tg, block, lds, s, a);
	else
		hipLaunchKernelGGL((k_synthesize_grid_ratio_transform<2>), tg, block, lds, s, a);
	if (a.q == 1) {
		const long long nq = (a.m_first + a.n_m - 1) / a.p - a.m_first / a.p + 1;
		const int per = (a.p < SGR_THREADS ? SGR_THREADS / a.p : 1) * SGR_S;
		const dim3 sg((unsigned)((nq + per - 1) / per));
		if (a.out_fmt == 0)
			hipLaunchKernelGGL((k_synthesize_grid_ratio_slide<0>), sg, block, 0, s, a);
		else
			hipLaunchKernelGGL((k_synthesize_grid_ratio_slide<2>), sg, block, 0, s, a);
	} else if (a.out_fmt == 0)
		hipLaunchKernelGGL((k_synthesize_grid_ratio_filter<0>), fg, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_synthesize_grid_ratio_filter<2>), fg, block, 0, s, a);
}

}  // namespace rx
