// grid_bank.h -- what the kernels of the channel grid share (DESIGN.md sections 4.19 - 4.21; include it behind dev_common.h): the tile
// of one workgroup, the launchers' dispatch on log2 M, the complex multiply and the two radix-2 butterflies, and the analysis bank:
// its branch sums and its decimation-in-frequency transform of length M = 2 D in LDS.  k_channelize_grid and k_survey_grid are
// grid_branch_sums + grid_dif + their own last step.  k_synthesize_grid_transform shares the tile, the butterfly and the dispatch and
// keeps the loops of its decimation-in-time transform in its own file: moved here they compiled to other code at M = 16, 32, 64 (13
// more instructions, 4 more VGPRs at M = 16) and the call at D = 8 measured about 1 % slower (profiles/grid_bank_parity.txt).  The
// headers of those files state the contracts.  The tile u[r][t] is time minor with rows of NT + 1 points.
#pragma once

namespace rx {

constexpr int GRID_THREADS = 256;
constexpr int GRID_HIST = 12;          // taps per branch sum: a = 0 .. 11, and a = 12 for branch 0 (T = 12 M + 1)
// times per tile: 4096 points of LDS, and never fewer than 8 times (64 bytes of a slot row, one group of the survey)
__host__ __device__ constexpr int grid_tile(int logm) { return (4096 >> logm) > 8 ? (4096 >> logm) : 8; }

// f(IntC<LOGM>{}) for the LOGM = 2 .. 10 of a launch, kernels.h's grid_logm(D) of a D the host has checked to be a power of two 2 ..
// 512 - the value must be exact: another logm launches nothing, and grid_logm of another D names a wrong instantiation.  A launcher
// keeps its own choice of the formats
template <class F> static void grid_dispatch(int logm, F f)
{
	switch (logm) {
	case 2: f(IntC<2>{}); break;
	case 3: f(IntC<3>{}); break;
	case 4: f(IntC<4>{}); break;
	case 5: f(IntC<5>{}); break;
	case 6: f(IntC<6>{}); break;
	case 7: f(IntC<7>{}); break;
	case 8: f(IntC<8>{}); break;
	case 9: f(IntC<9>{}); break;
	case 10: f(IntC<10>{}); break;
	}
}

__device__ __forceinline__ float2 grid_mul(float2 a, float2 w)
{
	return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * w.y)), __builtin_fmaf(a.x, w.y, a.y * w.x));
}
// one butterfly of a decimation-in-frequency stage whose root for this pair is w
__device__ __forceinline__ void grid_bfly_dif(float2 &p, float2 &q, float2 w)
{
	const float2 s = make_float2(p.x + q.x, p.y + q.y), d = make_float2(p.x - q.x, p.y - q.y);
	p = s;
	q = grid_mul(d, w);
}
// ... of a decimation-in-time stage
__device__ __forceinline__ void grid_bfly_dit(float2 &p, float2 &q, float2 w)
{
	const float2 b = grid_mul(q, w);
	q = make_float2(p.x - b.x, p.y - b.y);
	p = make_float2(p.x + b.x, p.y + b.y);
}

// work item `it` of a pass of the transform over 1 << LOGNB blocks of points and the tile's NT times: lanes along t where a tile has
// 64 times, else along b
template <int LOGNB, int NT> __device__ __forceinline__ void grid_item(int it, int &b, int &t)
{
	if (NT >= 64) {
		t = it & (NT - 1);
		b = it / NT;
	} else {
		b = it & ((1 << LOGNB) - 1);
		t = it >> LOGNB;
	}
}

// The branch sums of the tile whose first output time is n0 (absolute), into LDS: u_n[r] = sum_a h[r + M a] x[n D - r - M a], one FMA
// chain per component with a ascending; a position outside [a.in_first, a.in_first + a.n_in) is never loaded and enters as +0.  The
// input is read from global memory, lanes along r.  Times of one parity share their samples: with t = e + 2 s, sample a of time t is
// x[(n0 + e) D - r - M (a - s)], so a thread takes a run of CH times of one parity of its branch r and loads the CH + 12 samples
// j = a - s = -(CH - 1) .. 12 once each, newest first; sample j meets time s at tap a = j + s, and for a given s the taps still come
// in ascending a.  M < 256: 256 / M threads per branch, one run of 16 each; else the branches tid, tid + 256 .., both parities, runs
// of NT / 2.  Args: ChannelizeArgs or SurveyGridArgs (in, in_first, n_in, taps).  Ends with the barrier behind the last store.
template <int FMT, int LOGM, class Args> __device__ __forceinline__ void grid_branch_sums(float2 *u, const Args &a, long long n0, int tid)
{
	constexpr int M = 1 << LOGM, D = M / 2, NT = grid_tile(LOGM), NTS = NT + 1, HIST = GRID_HIST;
	constexpr int G = M < GRID_THREADS ? GRID_THREADS / M : 1;    // threads per branch
	constexpr int CH = M < GRID_THREADS ? 16 : NT / 2;            // times per run (G CH = NT, or 2 CH = NT)
	static_assert((G > 1 ? G * CH : 2 * CH) == NT, "the runs tile the times");
	const int g = M < GRID_THREADS ? tid >> LOGM : 0;
	for (int r = tid & (M < GRID_THREADS ? M - 1 : GRID_THREADS - 1); r < M; r += GRID_THREADS) {
		float h[HIST + 1];
		#pragma unroll
		for (int i = 0; i < HIST; ++i)
			h[i] = a.taps[r + M * i];
		h[HIST] = r == 0 ? a.taps[M * HIST] : 0.f;
		for (int run = 0; run < (G > 1 ? 1 : 2); ++run) {
			const int e = G > 1 ? g & 1 : run, s0 = G > 1 ? (g >> 1) * CH : 0;
			const int tf = e + 2 * s0;                                // the run's first time: t = tf + 2 s
			float re[CH], im[CH];
			#pragma unroll
			for (int s = 0; s < CH; ++s)
				re[s] = im[s] = 0.f;
			const long long m0 = (n0 + tf) * D - r - a.in_first;      // sample j = 0 of the run, counted from the buffer's first
			#pragma unroll
			for (int j = -(CH - 1); j <= HIST; ++j) {
				if (j == HIST && r != 0)                                  // tap a = 12 exists for branch 0 alone
					continue;
				const long long m = m0 - (long long)M * j;
				float2 x = make_float2(0.f, 0.f);
				if (m >= 0 && m < a.n_in)
					x = iq_sample<FMT>(a.in, (size_t)m);
				#pragma unroll
				for (int s = 0; s < CH; ++s) {
					const int i = j + s;                                  // the tap
					if (i < 0 || i > HIST || (i == HIST && r != 0))
						continue;
					re[s] = __builtin_fmaf(h[i], x.x, re[s]);
					im[s] = __builtin_fmaf(h[i], x.y, im[s]);
				}
			}
			#pragma unroll
			for (int s = 0; s < CH; ++s)
				u[r * NTS + tf + 2 * s] = make_float2(re[s], im[s]);
		}
	}
	__syncthreads();
}

// The transform of every time of the tile in place, decimation in frequency, two stages per pass over LDS: natural order in,
// bit-reversed out; tw[j] = e^{+2 pi i j / M}, j = 0 .. M / 2 - 1.  The stages of half-length M / 2, M / 4 .. 1 (the last alone when
// their number is odd); stage of half-length H: (p, q) = (x[i] + x[i + H], (x[i] - x[i + H]) w^{j M / (2 H)}), j = i mod H.  A pass
// takes the points i, i + Q, i + 2 Q, i + 3 Q (Q the second stage's half-length): stage 2 Q pairs (i, i + 2 Q) and (i + Q, i + 3 Q),
// stage Q pairs (i, i + Q) and (i + 2 Q, i + 3 Q).  The order of every sum is fixed by M alone.  A barrier ends every pass; the
// caller has one behind its last store to u.
template <int LOGM> __device__ __forceinline__ void grid_dif(float2 *u, const float2 *tw, int tid)
{
	constexpr int M = 1 << LOGM, NT = grid_tile(LOGM), NTS = NT + 1;
	#pragma unroll
	for (int lq = LOGM - 2; lq >= 0; lq -= 2) {
		const int Q = 1 << lq;
		for (int it = tid; it < (M / 4) * NT; it += GRID_THREADS) {
			int b, t;
			grid_item<LOGM - 2, NT>(it, b, t);
			const int j = b & (Q - 1), i = ((b >> lq) << (lq + 2)) + j;
			float2 *x = u + i * NTS + t;
			float2 x0 = x[0], x1 = x[Q * NTS], x2 = x[2 * Q * NTS], x3 = x[3 * Q * NTS];
			// stage 2 Q: the roots w^{j' M / (4 Q)} of j' = j and j + Q; stage Q: w^{j M / (2 Q)} for both pairs
			const float2 wa = tw[j << (LOGM - 2 - lq)], wb = tw[(j + Q) << (LOGM - 2 - lq)], wc = tw[j << (LOGM - 1 - lq)];
			grid_bfly_dif(x0, x2, wa);
			grid_bfly_dif(x1, x3, wb);
			grid_bfly_dif(x0, x1, wc);
			grid_bfly_dif(x2, x3, wc);
			x[0] = x0;
			x[Q * NTS] = x1;
			x[2 * Q * NTS] = x2;
			x[3 * Q * NTS] = x3;
		}
		__syncthreads();
	}
	if (LOGM & 1) {                                               // the stage of half-length 1: its root is 1
		for (int it = tid; it < (M / 2) * NT; it += GRID_THREADS) {
			int b, t;
			grid_item<LOGM - 1, NT>(it, b, t);
			float2 *x = u + 2 * b * NTS + t;
			float2 x0 = x[0], x1 = x[NTS];
			grid_bfly_dif(x0, x1, tw[0]);
			x[0] = x0;
			x[NTS] = x1;
		}
		__syncthreads();
	}
}

}  // namespace rx
