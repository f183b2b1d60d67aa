// k_synthesize_grid.hip -- the wideband synthesizer on a channel grid, the mirror image of
// k_channelize_grid.hip: a polyphase synthesis bank.  Interpolation D = 2, 4 .. 512, M = 2 D slots k = -M/2 .. M/2 - 1 with their
// centres at k rate / 2, the taps h of section 4.14 (T = 24 D + 1).  Row c belongs to slot k_c (pairwise distinct), starts at the
// wideband index start_c = sigma_c D and has the gain G_c = D gain_c:
//   w[m] = sum_c G_c e^{+2 pi i k_c m / M} sum_j h[m - start_c - j D] x_c[j],
// computed as
//   X_j[k_c mod M] = (-1)^{k_c j} (G_c x_c[j - sigma_c]),  every other entry +0                    (j: absolute input time)
//   V_j[r] = sum_k X_j[k] e^{+2 pi i k r / M},  r = 0 .. M - 1
//   w[q D + b] = sum_{a = 0 .. 23, and a = 24 where b = 0} h[b + a D] V_{q - a}[b + (a mod 2) D],  0 <= b < D;  V_j = 0 for j < 0.
// No NCO: the only irrational numbers are the transform's roots, which the host makes in double (a.tw, section 4.19's table).
// Two kernels, since an output meets V at 25 input times and one time is up to 8 KiB:
//   k_synthesize_grid_transform: one workgroup of 256 threads makes a tile of grid_tile(LOGM) input times in LDS, u[row][t] (time
//     minor, rows of NT + 1).  It clears the tile, places the rows' samples - lanes along time, so a row's loads are contiguous - at
//     row brev(k mod M), and runs the transform in place, decimation in time, radix 2, two stages per pass over LDS: bit-reversed
//     order in, natural order out.  Stage of half-length H: (p, q) = (x[i] + w x[i + H], x[i] - w x[i + H]), w = tw[j M / (2 H)],
//     j = i mod H.  The order of every sum is fixed by M alone.  V goes to the scratch as [time][r], r natural: the tile's M NT
//     points are one contiguous run, and the filter's lanes along b read 8 D contiguous bytes of a time.  A tile no row reaches
//     writes +0 and skips the rest (workgroup-uniform).
//   k_synthesize_grid_filter: work item (g, b) makes the SYG_R outputs (q0 + i) D + b, i = 0 .. SYG_R - 1, D apart: they share
//     their 24 (25) taps in registers and slide over the two V rows b and b + D of SYG_R + 24 times, newest first, so that every
//     output's chain runs with a ascending.  Lanes along b: loads and stores are contiguous along m.
// Contract on order: G_c x is one fp32 product; w is one FMA chain per component from +0, a ascending; every output passes through
// v + 0.f (iq_store).  No state: V_j is a function of j alone, so windows, tiles and the host's chunks change no byte.
#include "dev_common.h"
#include "grid_bank.h"
#include "kernels.h"

namespace rx {

constexpr int SYG_HIST = 24;

template <int IFMT, int LOGM>
__global__ __launch_bounds__(GRID_THREADS) void k_synthesize_grid_transform(SynthesizeGridArgs a)
{
	constexpr int M = 1 << LOGM, NT = grid_tile(LOGM), NTS = NT + 1;
	__shared__ float2 u[M * NTS];
	const int tid = threadIdx.x;
	const int t0 = blockIdx.x * NT;                               // the tile's first time in the scratch
	const long long j0 = a.j_first + t0;                          // ... as an absolute input time (may be negative: V is zero there)
	float2 *dst = a.scratch + (size_t)t0 * M;                     // the tile's M NT points, [time][r]: index t M + r

	// does any row reach the tile?  Row c holds the times sigma_c .. sigma_c + n_in - 1
	int hit = 0;
	for (int c = tid; c < a.n_channels; c += GRID_THREADS) {
		const long long sg = a.ch[c].start >> (LOGM - 1);
		hit |= sg <= j0 + NT - 1 && sg + a.n_in - 1 >= j0;
	}
	if (!__syncthreads_or(hit)) {
		for (int it = tid; it < M * NT; it += GRID_THREADS)
			dst[it] = make_float2(0.f, 0.f);
		return;
	}

	// ---- 1. X: zeros, then the rows' samples at row brev(k mod M); (-1)^{k j}.  The slots are distinct: no two items share a point
	for (int it = tid; it < M * NTS; it += GRID_THREADS)
		u[it] = make_float2(0.f, 0.f);
	__syncthreads();
	for (int it = tid; it < a.n_channels * NT; it += GRID_THREADS) {
		const int t = it & (NT - 1), c = it / NT;
		const SynthChannel ch = a.ch[c];
		const long long j = j0 + t, i = j - (ch.start >> (LOGM - 1));
		if (i < 0 || i >= a.n_in)
			continue;
		const float2 x = iq_sample<IFMT>(a.in, (size_t)c * (size_t)a.in_stride + (size_t)i);
		float2 v = make_float2(ch.gain * x.x, ch.gain * x.y);
		const unsigned k = ch.inc >> (32 - LOGM);                     // inc = k 2^32 / M mod 2^32
		if (k & (unsigned)j & 1u)
			v = make_float2(-v.x, -v.y);
		u[(__brev(k) >> (32 - LOGM)) * NTS + t] = v;
	}
	__syncthreads();

	// ---- 2. the transform: the stages of half-length 1, 2 .. M / 2 (the first alone when their number is odd), then two per pass.
	// A pass takes the points i, i + Q, i + 2 Q, i + 3 Q: stage Q pairs (i, i + Q) and (i + 2 Q, i + 3 Q), stage 2 Q pairs
	// (i, i + 2 Q) and (i + Q, i + 3 Q).  Work item (b, t): lanes along t where a tile has 64 times.  (The mirror image of
	// grid_bank.h's grid_dif; why the loops stand here and not there is said in that header)
	const float2 *tw = a.tw;
	if (LOGM & 1) {                                               // the stage of half-length 1: its root is 1
		for (int it = tid; it < (M / 2) * NT; it += GRID_THREADS) {
			int b, t;
			if (NT >= 64) {
				t = it & (NT - 1);
				b = it / NT;
			} else {
				b = it & (M / 2 - 1);
				t = it >> (LOGM - 1);
			}
			float2 *x = u + 2 * b * NTS + t;
			float2 x0 = x[0], x1 = x[NTS];
			grid_bfly_dit(x0, x1, tw[0]);
			x[0] = x0;
			x[NTS] = x1;
		}
		__syncthreads();
	}
	#pragma unroll
	for (int lq = LOGM & 1; lq <= LOGM - 2; lq += 2) {
		const int Q = 1 << lq;
		for (int it = tid; it < (M / 4) * NT; it += GRID_THREADS) {
			int b, t;
			if (NT >= 64) {
				t = it & (NT - 1);
				b = it / NT;
			} else {
				b = it & (M / 4 - 1);
				t = it >> (LOGM - 2);
			}
			const int j = b & (Q - 1), i = ((b >> lq) << (lq + 2)) + j;
			float2 *x = u + i * NTS + t;
			float2 x0 = x[0], x1 = x[Q * NTS], x2 = x[2 * Q * NTS], x3 = x[3 * Q * NTS];
			// stage Q: w^{j M / (2 Q)} for both pairs; stage 2 Q: the roots w^{j' M / (4 Q)} of j' = j and j + Q
			const float2 wc = tw[j << (LOGM - 1 - lq)], wa = tw[j << (LOGM - 2 - lq)], wb = tw[(j + Q) << (LOGM - 2 - lq)];
			grid_bfly_dit(x0, x1, wc);
			grid_bfly_dit(x2, x3, wc);
			grid_bfly_dit(x0, x2, wa);
			grid_bfly_dit(x1, x3, wb);
			x[0] = x0;
			x[Q * NTS] = x1;
			x[2 * Q * NTS] = x2;
			x[3 * Q * NTS] = x3;
		}
		__syncthreads();
	}

	// ---- 3. V to the scratch: point t M + r is row r, time t of the tile
	for (int it = tid; it < M * NT; it += GRID_THREADS)
		dst[it] = u[(it & (M - 1)) * NTS + (it >> LOGM)];
}

// outputs per work item, D apart; work items per tile: one per b, and 256 / D groups where D < 256
constexpr int SYG_R = 8;
__host__ __device__ constexpr int syg_groups(int logm) { return (1 << (logm - 1)) < GRID_THREADS ? GRID_THREADS >> (logm - 1) : 1; }

template <int OFMT, int LOGM>
__global__ __launch_bounds__(GRID_THREADS) void k_synthesize_grid_filter(SynthesizeGridArgs a)
{
	constexpr int M = 1 << LOGM, D = M / 2, G = syg_groups(LOGM), QT = G * SYG_R, R = SYG_R;
	const long long out_hi = a.out_first + a.n_out;
	for (int item = threadIdx.x; item < G * D; item += GRID_THREADS) {
		const int g = item >> (LOGM - 1), b = item & (D - 1);
		const int qs = blockIdx.x * QT + g * R;                       // the item's first output time, counted from the chunk's first
		if (qs >= a.nq)
			continue;
		float h[SYG_HIST + 1];
		#pragma unroll
		for (int k = 0; k < SYG_HIST; ++k)
			h[k] = a.taps[b + k * D];
		h[SYG_HIST] = b == 0 ? a.taps[SYG_HIST * D] : 0.f;
		float wr[R], wi[R];
		#pragma unroll
		for (int i = 0; i < R; ++i)
			wr[i] = wi[i] = 0.f;
		// scratch time of absolute time j: j - (q_first - 24); the item's newest time is qs + R - 1 + 24 there
		const float2 *v = a.scratch + (size_t)(qs + R - 1 + SYG_HIST) * M + b;
		#pragma unroll
		for (int jj = 0; jj < R + SYG_HIST; ++jj) {                   // time q0 + R - 1 - jj: output i meets it at tap a = jj - (R - 1 - i)
			const float2 ve = v[-(ptrdiff_t)jj * M], vo = v[-(ptrdiff_t)jj * M + D];
			#pragma unroll
			for (int i = 0; i < R; ++i) {
				const int t = jj - (R - 1 - i);
				if (t < 0 || t > SYG_HIST)
					continue;
				const float2 x = (t & 1) ? vo : ve;
				if (t < SYG_HIST) {
					wr[i] = __builtin_fmaf(h[t], x.x, wr[i]);
					wi[i] = __builtin_fmaf(h[t], x.y, wi[i]);
				} else {                                                  // tap a = 24 exists for b = 0 alone
					wr[i] = b == 0 ? __builtin_fmaf(h[t], x.x, wr[i]) : wr[i];
					wi[i] = b == 0 ? __builtin_fmaf(h[t], x.y, wi[i]) : wi[i];
				}
			}
		}
		#pragma unroll
		for (int i = 0; i < R; ++i) {
			const long long m = (a.q_first + qs + i) * D + b;
			if (qs + i >= a.nq || m < a.out_first || m >= out_hi)
				continue;
			iq_store<OFMT>(a.out, m - a.out_first, 0, wr[i], wi[i]);     // (-0 -> +0: see k_synthesize.hip's header)
		}
	}
}

int synthesize_grid_tile_times(int interp) { return grid_tile(grid_logm(interp)); }
int synthesize_grid_filter_times(int interp) { return syg_groups(grid_logm(interp)) * SYG_R; }

template <int IFMT, int OFMT> static void syg_launch(hipStream_t s, const SynthesizeGridArgs &a)
{
	grid_dispatch(grid_logm(a.p), [&](auto c) {
		constexpr int LOGM = decltype(c)::value, QT = syg_groups(LOGM) * SYG_R;
		hipLaunchKernelGGL((k_synthesize_grid_transform<IFMT, LOGM>), dim3((unsigned)(a.n_times / grid_tile(LOGM))), dim3(GRID_THREADS), 0, s, a);
		hipLaunchKernelGGL((k_synthesize_grid_filter<OFMT, LOGM>), dim3((unsigned)((a.nq + QT - 1) / QT)), dim3(GRID_THREADS), 0, s, a);
	});
}

void launch_synthesize_grid(hipStream_t s, const SynthesizeGridArgs &a)
{
	if (a.in_fmt == 0 && a.out_fmt == 0)
		syg_launch<0, 0>(s, a);
	else if (a.in_fmt == 0)
		syg_launch<0, 2>(s, a);
	else if (a.out_fmt == 0)
		syg_launch<2, 0>(s, a);
	else
		syg_launch<2, 2>(s, a);
}

}  // namespace rx
