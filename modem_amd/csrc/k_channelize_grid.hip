// k_channelize_grid.hip -- the wideband front end on a channel grid: a polyphase filter bank.  Decimation
// D = 2, 4 .. 512, M = 2 D slots k = -M/2 .. M/2 - 1 with their centres at k rate / 2, the taps h of section 4.14 (T = 12 M + 1):
//   y_k[n] = sum_{t = 0 .. T - 1} h[t] x[n D - t] e^{-2 pi i k (n D - t) / M},   x zero outside the buffer,
// computed as
//   u_n[r] = sum_a h[r + M a] x[n D - r - M a],  r = 0 .. M - 1,  a = 0 .. 11 (and a = 12 for r = 0),
//   y_k[n] = (-1)^{k n} sum_r u_n[r] e^{+2 pi i k r / M}:  one pass of the filter for all slots, one inverse DFT of length M per
// output time, a sign.  No NCO: the only irrational numbers are the transform's roots, which the host makes in double (a.tw).
// One workgroup of 256 threads makes a tile of NT output times (steps 1 and 2 are grid_bank.h's, shared with k_survey_grid.hip):
//   1. the branch sums of the tile into LDS, u[r][t] (time minor, rows of NT + 1).  The input is read from global memory, lanes along
//      r: 64 neighbouring sample frames per load.  Output times of one parity share their samples (n D and (n + 2) D lie M apart), so
//      a thread forms a run of 4 .. 16 such times of one branch from one pass over their samples in registers: 1.75 (D <= 64) to 4
//      (D = 512) loads per branch sum, not 12; what is left of the 24 times a sample enters meets it again in L1 / L2 (at D = 512
//      the span of a tile of 8 times is 134 KiB as fp32 - there is no room to stage it in LDS beside the tile);
//   2. the transform in place, decimation in frequency, radix 2, two stages per pass over LDS: natural order in, bit-reversed out.
//      Stage of half-length H: (p, q) = (x[i] + x[i + H], (x[i] - x[i + H]) w^{j M / (2 H)}), j = i mod H.  The order of every sum is
//      fixed by M alone, so an output does not depend on the tile, the launch or the block it belongs to;
//   3. the requested slots only: row brev(k mod M) of the tile, the sign, NT neighbouring outputs of one slot row per NT lanes - at
//      least 64 contiguous bytes per row.
// Contract on order: u_n[r] is one FMA chain per component, a ascending; a position outside [in_first, in_first + n_in) is never
// loaded and enters as +0.  No state: a capture cut into blocks, each with the T - 1 samples before it, gives the bytes of one call.
#include "dev_common.h"
#include "grid_bank.h"
#include "kernels.h"

namespace rx {

template <int FMT, int LOGM>
__global__ __launch_bounds__(GRID_THREADS) void k_channelize_grid(ChannelizeArgs a)
{
	constexpr int M = 1 << LOGM, NT = grid_tile(LOGM), NTS = NT + 1;
	__shared__ float2 u[M * NTS];
	const int tid = threadIdx.x;
	const long long j0 = (long long)blockIdx.x * NT;              // the tile's first output, counted from out_first
	const long long n0 = a.out_first + j0;
	const int nt = (int)(a.n_out - j0 < NT ? a.n_out - j0 : NT);  // output times of the tile that exist

	// ---- 1. the branch sums, 2. the transform: u[brev(k mod M)][t] = sum_r u_n[r] e^{+2 pi i k r / M}
	grid_branch_sums<FMT, LOGM>(u, a, n0, tid);
	grid_dif<LOGM>(u, a.tw, tid);

	// ---- 3. the requested slots: slot k's sum stands in row brev(k mod M); (-1)^{k n}
	for (int it = tid; it < a.n_channels * NT; it += GRID_THREADS) {
		const int t = it & (NT - 1), c = it / NT;
		if (t >= nt)
			continue;
		const unsigned k = a.inc[c] >> (32 - LOGM);                   // inc = k 2^32 / M mod 2^32
		const unsigned row = __brev(k) >> (32 - LOGM);
		float2 v = u[row * NTS + t];
		if (k & (unsigned)(n0 + t) & 1u)
			v = make_float2(-v.x, -v.y);
		float2 *dst = a.dst ? (float2 *)(uintptr_t)a.dst[c] : (float2 *)a.out + (size_t)c * (size_t)a.out_stride;
		dst[j0 + t] = v;
	}
}

template <int FMT> static void chg_launch(hipStream_t s, const ChannelizeArgs &a)
{
	grid_dispatch(grid_logm(a.p), [&](auto c) {
		constexpr int LOGM = decltype(c)::value, NT = grid_tile(LOGM);
		hipLaunchKernelGGL((k_channelize_grid<FMT, LOGM>), dim3((unsigned)((a.n_out + NT - 1) / NT)), dim3(GRID_THREADS), 0, s, a);
	});
}

// (the shortest tile is 8 output times: the grid's x stays below 2^31)
long long channelize_grid_max_outputs() { return 8LL * 0x7fffffffLL; }

void launch_channelize_grid(hipStream_t s, const ChannelizeArgs &a)
{
	if (a.fmt == 0)
		chg_launch<0>(s, a);
	else if (a.fmt == 1)
		chg_launch<1>(s, a);
	else
		chg_launch<2>(s, a);
}

}  // namespace rx
