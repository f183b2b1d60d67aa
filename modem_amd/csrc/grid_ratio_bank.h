// grid_ratio_bank.h -- what the kernels of the channel grid at a ratio share (DESIGN.md sections 4.22 and 4.24; include it behind
// dev_common.h and grid_bank.h): the analysis bank of M = 2 P = 2^a 3^b 5^c points - its branch sums with the tap phase of every
// output time and its mixed-radix decimation-in-frequency transform in LDS.  k_channelize_grid_ratio and k_survey_grid_ratio are
// cgr_branch_sums + cgr_transform + their own last step, so both hold the same bytes in LDS for the same output time; the header of
// k_channelize_grid_ratio.hip states the contract.  The tile u[r][t] is time minor with rows of NT + 1 points; NT is the caller's (the
// order of every sum is fixed by M and by absolute indices, never by the tile).  The synthesizer (k_synthesize_grid_ratio.hip) runs
// the transform the other way and keeps its own loops.
#pragma once

namespace rx {

constexpr int CGR_THREADS = 256;
constexpr int CGR_HIST = 13;           // taps per branch at most: T <= 12 M + 1

// grid_bank.h's multiply on a cf
__device__ __forceinline__ cf cgr_mul(cf a, float2 w)
{
	const float2 v = grid_mul(make_float2(a.re, a.im), w);
	return mk(v.x, v.y);
}

// one stage of radix R on blocks of N points, every time of the tile
template <int R> __device__ __forceinline__ void cgr_stage(cf *u, const float2 *tw, int tid, int M, int N, int NT)
{
	const int NTS = NT + 1, L = N / R, step = M / N, nb = M / R;
	for (int it = tid; it < nb * NT; it += CGR_THREADS) {
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
		Bfly<R>::run(v);
		if (L > 1) {
			#pragma unroll
			for (int i = 1; i < R; ++i)
				v[i] = cgr_mul(v[i], tw[j * i * step]);
		}
		#pragma unroll
		for (int i = 0; i < R; ++i)
			x[i * L * NTS] = v[i];
	}
	__syncthreads();
}

// The branch sums of the tile of NT times whose first output time is n0 (absolute), into LDS.  Work item (r, e, g): branch r, the run
// of times t = tf + 2 Q s < NT, tf = e + 2 Q CH g (ns <= CH of them).  Time s stands at i_tf + M s with the phase of tf, so sample a of
// time s is x[i_tf - r - M (a - s)]: the run loads the samples j = a - s = -(ns - 1) .. na - 1 once each, newest first; sample j meets
// time s at tap a = j + s, and for a given s the taps still come in ascending a.  (The plan picks CH so that a small M still gives
// every thread a run.)  Args: ChannelizeArgs or SurveyGridRatioArgs (in, in_first, n_in, p, q, taps).  The caller puts a barrier
// behind it.
template <int FMT, int CH, class Args>
__device__ __forceinline__ void cgr_branch_sums(cf *u, const Args &a, int M, int NT, int T, int groups, long long n0, int tid)
{
	const int NTS = NT + 1, Q = a.q, Q2 = 2 * a.q;
	const int E = Q2 < NT ? Q2 : NT;
	for (int w = tid; w < M * E * groups; w += CGR_THREADS) {
		const int eg = w / M, r = w - eg * M, g = eg / E, e = eg - g * E;
		const int tf = e + Q2 * CH * g;                               // the run's first time
		if (tf >= NT)
			continue;
		const long long un = (n0 + tf) * a.p, i0 = un / Q;
		const int ph = (int)(un - i0 * Q);
		const int na = r < T ? (T - 1 - r) / M + 1 : 0;           // the taps r + M a <= T - 1 of the branch
		const int left = (NT - tf + Q2 - 1) / Q2, ns = left < CH ? left : CH;
		float h[CGR_HIST];
		#pragma unroll
		for (int i = 0; i < CGR_HIST; ++i)
			h[i] = i < na ? a.taps[(size_t)(r + M * i) * Q + ph] : 0.f;
		float re[CH], im[CH];
		#pragma unroll
		for (int s = 0; s < CH; ++s)
			re[s] = im[s] = 0.f;
		const long long m0 = i0 - r - a.in_first;                 // sample j = 0 of the run, counted from the buffer's first
		#pragma unroll
		for (int j = -(CH - 1); j < CGR_HIST; ++j) {
			if (j >= na || j + ns <= 0)
				continue;
			const long long m = m0 - (long long)M * j;
			float2 x = make_float2(0.f, 0.f);
			if (m >= 0 && m < a.n_in)
				x = iq_sample<FMT>(a.in, (size_t)m);
			#pragma unroll
			for (int s = 0; s < CH; ++s) {
				const int i = j + s;                                  // the tap
				if (i < 0 || i >= CGR_HIST)
					continue;
				if (i < na && s < ns) {
					re[s] = __builtin_fmaf(h[i], x.x, re[s]);
					im[s] = __builtin_fmaf(h[i], x.y, im[s]);
				}
			}
		}
		#pragma unroll
		for (int s = 0; s < CH; ++s)
			if (s < ns)
				u[r * NTS + tf + Q2 * s] = mk(re[s], im[s]);
	}
}

// the transform in place: the plan's radices, four bits each, first stage lowest.  A barrier ends every stage
__device__ __forceinline__ void cgr_transform(cf *u, const float2 *tw, unsigned radices, int tid, int M, int NT)
{
	int N = M;
	#pragma unroll
	for (int s = 0; s < 8; ++s) {
		const int R = (int)((radices >> (4 * s)) & 15u);
		if (R == 0)
			break;
		switch (R) {
		case 5: cgr_stage<5>(u, tw, tid, M, N, NT); break;
		case 3: cgr_stage<3>(u, tw, tid, M, N, NT); break;
		case 4: cgr_stage<4>(u, tw, tid, M, N, NT); break;
		default: cgr_stage<2>(u, tw, tid, M, N, NT); break;
		}
		N /= R;
	}
}

}  // namespace rx
