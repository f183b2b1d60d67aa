// k_stream.hip -- the stream scan: every Schmidl-Cox preamble of a long recording (decode.cc:84-151 over the whole stream), with
// all CUs on it.  No stage walks the stream in one wave or one workgroup:
//   k_sdc_tile / k_sdcs_scan  mono input: the DC blocker's kept states (k_mono_carries' layout) by tiles from a zero state, a scan of
//                             the tile carries with the a^4096 weights, and a fix-up
//   k_stream_tile<.., false>  per tile of STREAM_TILE sample times: the timing metric (decode.cc:86-90) from window sums the tile
//                             forms itself in double, then what the tile does to the trigger state for either incoming Schmitt state
//   k_streams_fn_scan         one workgroup per recording scans those per-tile functions (a tile is 4096 samples: 1/4096 of the stream)
//   k_stream_tile<.., true>   the tiles again, now with their incoming state: falling edges, t_max, index_max, in stream order
//   k_stream_accept           decode.cc:110-151 for every edge (sc_accept_wg, shared with k_sync_accept)
//   k_streams_count / _first / _records   a scan over accept / reject: record indices, cumulative rejects, the SyncState of every
//                             record, at its place in the packed order of the call's recordings
// Recordings (api_streams.cpp; one recording is a batch of one): the FB = SourceBatch forms take the recording
// from blockIdx.y - its own base, length and places in the per-tile and edge arrays; the scans over tiles are one workgroup per
// recording, so nothing is carried from one recording into the next.
// Live channels (api_bank.cpp; a feed is a bank of one channel) run the same kernels push by push over a
// window of every channel's stream: the FB = WindowBatch forms take the channel from blockIdx.y - where the push's first tile / block
// lies in its stream and the state its last push left - and compute from the same absolute positions as a recording's scan.
#include <type_traits>
#include "dev_common.h"
#include "kernels.h"
#include "mono_front.h"
#include "sync_accept.h"

namespace rx {

template <class FB> constexpr bool many_v = std::is_same<FB, SourceBatch>::value;
template <class FB> constexpr bool bank_v = std::is_same<FB, WindowBatch>::value;   // many live channels

// inclusive Hillis-Steele scan over NT threads in LDS (sh: NT entries); returns this thread's inclusive value, sh holds them all
// afterwards (the caller synchronises before reusing sh)
template <int NT, class T, class Op>
__device__ __forceinline__ T block_scan_incl(T v, T *sh, int tid, Op op)
{
	sh[tid] = v;
	__syncthreads();
	for (int k = 1; k < NT; k <<= 1) {
		T o = sh[tid >= k ? tid - k : 0];
		__syncthreads();
		if (tid >= k) {
			v = op(o, v);
			sh[tid] = v;
		}
		__syncthreads();
	}
	return v;
}

// ---------------------------------------------------------------- mono: the DC blocker over the whole stream
struct Affine { double v, w; };                               // x -> w x + v
__device__ __forceinline__ Affine aff_then(Affine l, Affine r) { return Affine{ r.v + r.w * l.v, l.w * r.w }; }

// PASS 0: the state each tile ends on from a zero state; PASS 1: the kept states from the tile's true entry state tile_in[t]
// FB = SourceBatch: tile blockIdx.x of recording blockIdx.y; ck_n is then the states kept per recording (the row length of ck)
// FB = WindowBatch (live channels): tile 0 of channel blockIdx.y starts at the absolute position fb.dc_from[q] (a
// multiple of MONO_CK), the channel's samples and states are addressed from where position 0 / state 0 would lie, fb.len[q] is the
// samples fed so far; only the states of complete blocks of MONO_CK samples are kept (ck_n is unused)
template <int PASS, class FB>
__global__ __launch_bounds__(256) void k_sdc_tile(FB fb, FrontCoef co, double *__restrict__ tile_end, const double *__restrict__ tile_in,
	double *__restrict__ ck, int ck_n)
{
	static_assert(many_v<FB> || bank_v<FB>, "recordings or live channels");
	long origin = 0;
	const int tid = threadIdx.x;
	const long t = blockIdx.x;
	MonoFrame fr{ (const char *)fb.samples, fb.fmt, fb.samples_per_frame, nullptr };
	if constexpr (many_v<FB>) {
		const int q = blockIdx.y;
		fr.base += (size_t)q * fb.frame_stride_bytes;
		fr.n = fb.src_len[q];
		if (t * 4096 >= fr.n)                                     // (uniform: a tile past this recording's end)
			return;
		tile_end += fb.tile0[q];
		tile_in += fb.tile0[q];
		ck += (size_t)q * ck_n;
		ck_n = (int)((fr.n + MONO_CK - 1) / MONO_CK);               // (mono_ck_per_frame)
	}
	if constexpr (bank_v<FB>) {                                   // channel blockIdx.y: its window, its tiles from where its DC blocker stands
		const int q = blockIdx.y;
		if ((long long)t >= fb.dc_at[q + 1] - fb.dc_at[q])          // (uniform)
			return;
		fr.base = batch_base(fb, q);
		fr.n = (long)fb.len[q];
		tile_end += fb.dc_at[q];
		tile_in += fb.dc_at[q];
		ck = (double *)((char *)ck + fb.ck_org[q]);
		origin = (long)fb.dc_from[q];
	}
	__shared__ Affine sh[256];
	const double a = (double)co.dc_a, g = (double)co.dc_b * (1.0 - a) * (double)fr.scale();
	const long s0 = (bank_v<FB> ? origin : 0) + t * 4096 + (long)tid * 16;
	double sl = 0.0;
	float x8[8];
	fr.load8(s0, x8);
	for (int i = 0; i < 8; ++i)
		sl = a * sl + g * (double)x8[i];
	fr.load8(s0 + 8, x8);
	for (int i = 0; i < 8; ++i)
		sl = a * sl + g * (double)x8[i];
	const Affine me = block_scan_incl<256>(Affine{ sl, mono_pow(a, 16) }, sh, tid, aff_then);
	if (PASS == 0) {
		if (tid == 255)
			tile_end[t] = me.v;
	} else {
		const double s_true = me.v + mono_pow(a, 16 * (tid + 1)) * tile_in[t];
		const long m = (bank_v<FB> ? origin / MONO_CK : 0) + t * (4096 / MONO_CK) + (tid >> 2);    // this thread ends sample 16 tid + 15 of its tile
		if ((tid & 3) == 3 && (bank_v<FB> ? (m + 1) * MONO_CK <= fr.n : m < ck_n))
			ck[m] = s_true;
	}
}

// the tiles' entry states C_0 = 0, C_{t+1} = tile_end[t] + a^4096 C_t: one workgroup per recording, on that recording's tiles -
// a range of tiles per thread composed as an affine map, an exclusive scan of the maps, then each range in turn.  The ranges per
// thread and the order of composition depend on the recording's own tile count alone, so a recording's doubles are the same
// whatever else the call holds.
__global__ __launch_bounds__(1024) void k_sdcs_scan(FrontCoef co, const double *__restrict__ tile_end_all, double *__restrict__ tile_in_all,
	const long long *__restrict__ tile0)
{
	const int tid = threadIdx.x;
	__shared__ Affine sh[1024];
	const double *__restrict__ tile_end = tile_end_all + tile0[blockIdx.x];
	double *__restrict__ tile_in = tile_in_all + tile0[blockIdx.x];
	const long ntiles = (long)(tile0[blockIdx.x + 1] - tile0[blockIdx.x]);
	const double A = mono_pow((double)co.dc_a, 4096);
	const long per = (ntiles + 1023) / 1024, k0 = (long)tid * per, k1 = k0 + per < ntiles ? k0 + per : ntiles;
	Affine f{ 0.0, 1.0 };
	for (long k = k0; k < k1; ++k)
		f = aff_then(f, Affine{ tile_end[k], A });
	block_scan_incl<1024>(f, sh, tid, aff_then);
	double c = tid ? sh[tid - 1].v : 0.0;                     // the maps applied to C_0 = 0
	for (long k = k0; k < k1; ++k) {
		tile_in[k] = c;
		c = tile_end[k] + A * c;
	}
}

// Many live channels: one workgroup per channel runs k_sdcs_scan's scan on the tiles that channel brings in this push - the same
// ranges per thread, the same order of composition whatever the other channels bring, so the same doubles - with the maps applied
// to the state kept before the channel's first tile (left by its earlier pushes) instead of 0.
__global__ __launch_bounds__(1024) void k_bank_sdc_scan(WindowBatch fb, FrontCoef co, const double *__restrict__ tile_end_all, double *__restrict__ tile_in_all,
	const double *__restrict__ ck_all)
{
	const int tid = threadIdx.x, q = blockIdx.x;
	__shared__ Affine sh[1024];
	const long ntiles = (long)(fb.dc_at[q + 1] - fb.dc_at[q]);
	if (ntiles == 0)                                              // (uniform)
		return;
	const double *__restrict__ tile_end = tile_end_all + fb.dc_at[q];
	double *__restrict__ tile_in = tile_in_all + fb.dc_at[q];
	const double *ck = (const double *)((const char *)ck_all + fb.ck_org[q]);
	const double *entry = fb.dc_from[q] > 0 ? ck + fb.dc_from[q] / MONO_CK - 1 : nullptr;
	const double A = mono_pow((double)co.dc_a, 4096);
	const long per = (ntiles + 1023) / 1024, k0 = (long)tid * per, k1 = k0 + per < ntiles ? k0 + per : ntiles;
	Affine f{ 0.0, 1.0 };
	for (long k = k0; k < k1; ++k)
		f = aff_then(f, Affine{ tile_end[k], A });
	block_scan_incl<1024>(f, sh, tid, aff_then);
	const double c0 = entry ? *entry : 0.0;                       // the maps applied to C_0 = the entry state
	double c = tid ? sh[tid - 1].v + sh[tid - 1].w * c0 : c0;
	for (long k = k0; k < k1; ++k) {
		tile_in[k] = c;
		c = tile_end[k] + A * c;
	}
}

void launch_streams_dc(hipStream_t s, int n_src, long max_len, SourceBatch fb, FrontCoef co, double *tile_end, double *tile_in, double *ck, int ck_per_src)
{
	const dim3 grid((unsigned)((max_len + 4095) / 4096), (unsigned)n_src);
	hipLaunchKernelGGL((k_sdc_tile<0, SourceBatch>), grid, dim3(256), 0, s, fb, co, tile_end, tile_in, ck, ck_per_src);
	hipLaunchKernelGGL(k_sdcs_scan, dim3((unsigned)n_src), dim3(1024), 0, s, co, tile_end, tile_in, fb.tile0);
	hipLaunchKernelGGL((k_sdc_tile<1, SourceBatch>), grid, dim3(256), 0, s, fb, co, tile_end, tile_in, ck, ck_per_src);
}
void launch_bank_dc(hipStream_t s, int n_ch, long max_tiles, WindowBatch fb, FrontCoef co, double *tile_end, double *tile_in, double *ck)
{
	const dim3 grid((unsigned)max_tiles, (unsigned)n_ch);
	hipLaunchKernelGGL((k_sdc_tile<0, WindowBatch>), grid, dim3(256), 0, s, fb, co, tile_end, tile_in, ck, 0);
	hipLaunchKernelGGL(k_bank_sdc_scan, dim3((unsigned)n_ch), dim3(1024), 0, s, fb, co, tile_end, tile_in, ck);
	hipLaunchKernelGGL((k_sdc_tile<1, WindowBatch>), grid, dim3(256), 0, s, fb, co, tile_end, tile_in, ck, 0);
}

// ---------------------------------------------------------------- the trigger as a scan
// comb: the running maximum of decode.cc:99-102 - the earlier one (l) keeps a tie
__device__ __forceinline__ void comb(float &m, long long &i, float m2, long long i2)
{
	if (m < m2) {
		m = m2;
		i = i2;
	}
}
struct Seg { int has; float m; long long i; };                // since the last falling edge (has: there was one)
__device__ __forceinline__ Seg seg_then(Seg l, Seg r)
{
	if (r.has)
		return r;
	Seg o = l;
	comb(o.m, o.i, r.m, r.i);
	return o;
}
__device__ __forceinline__ int last_then(int l, int r) { return r >= 0 ? r : l; }
__device__ __forceinline__ long long add_ll(long long l, long long r) { return l + r; }

struct TrigShared {
	int last[256];
	Seg seg[256];
	long long cnt[256];
};
constexpr int SPT = STREAM_TILE / 256;                        // sample times per thread

// The tile's trigger given the state entering it (s_in, running maximum m_in / i_in).  cls: +1 above hi (sets), -1 below lo (clears),
// 0 holds (and every time at or past the end of the stream).  Out: the state entering this thread, the running maximum entering it,
// the falling edges of the threads before it; tile totals in *s_out / *seg_out / *n_out (every thread).
__device__ __forceinline__ void tile_trigger(TrigShared &sh, const int (&cls)[SPT], const float (&v)[SPT], long long t0, int tid,
	int s_in, float m_in, long long i_in, int &s_thr, Seg &seg_thr, long long &edges_before, int &s_out, Seg &seg_out, long long &n_out)
{
	int last = -1;
	for (int j = 0; j < SPT; ++j)
		if (cls[j])
			last = cls[j] > 0;
	const int incl = block_scan_incl<256>(last, sh.last, tid, last_then);
	const int excl = tid ? sh.last[tid - 1] : -1;
	s_thr = excl >= 0 ? excl : s_in;
	const int tile_last = sh.last[255];
	s_out = tile_last >= 0 ? tile_last : s_in;
	(void)incl;
	__syncthreads();
	int s = s_thr;
	Seg mine{ 0, -INFINITY, -1 };
	long long ne = 0;
	for (int j = 0; j < SPT; ++j) {
		if (cls[j] < 0 && s == 1) {                               // a falling edge: its run ends here (the edge sample belongs to it)
			++ne;
			mine = Seg{ 1, -INFINITY, -1 };
		} else {
			comb(mine.m, mine.i, v[j], t0 + j);
		}
		if (cls[j])
			s = cls[j] > 0;
	}
	block_scan_incl<256>(mine, sh.seg, tid, seg_then);
	const Seg before = tid ? sh.seg[tid - 1] : Seg{ 0, -INFINITY, -1 };
	seg_thr = seg_then(Seg{ 0, m_in, i_in }, before);
	seg_out = seg_then(Seg{ 0, m_in, i_in }, sh.seg[255]);
	__syncthreads();
	block_scan_incl<256>(ne, sh.cnt, tid, add_ll);
	edges_before = tid ? sh.cnt[tid - 1] : 0;
	n_out = sh.cnt[255];
	__syncthreads();
}

// EMIT = false: the timing metric of the tile and its function (StreamFn) for both incoming states; EMIT = true: the same metric and
// the tile's falling edges from its incoming StreamCarry.  GIVEN: the metric is a caller's sequence (ofdmrx_debug_streams_edges).
// FB = SourceBatch: tile blockIdx.x of recording blockIdx.y, read from that recording's base with its length (n is unused): a position
// below 0 or at or past the length reads as zero, whatever lies behind the recording; edges is [recordings][cap]
// FB = WindowBatch: block b of the live channel q = blockIdx.y is tile fb.tile0[q] + b of its stream - the same absolute sample
// positions as in a recording's scan, so the same metric values - read from where the channel's position 0 would lie, with the samples
// fed so far as its length (n is unused); fn / carry are indexed from fb.tile_at[q], edges is [channels][cap], and the edge positions
// count from the push's first edge (the carry that enters a push has count 0)
template <int RATE, bool GIVEN, bool EMIT, class FB>
__global__ __launch_bounds__(256) void k_stream_tile(FB fb, const float *__restrict__ given, long n, StreamFn *__restrict__ fn,
	const StreamCarry *__restrict__ carry, StreamEdge *__restrict__ edges, long cap)
{
	static_assert(many_v<FB> || bank_v<FB>, "recordings or live channels");
	const void *samples = fb.samples;
	long long tile0 = 0;
	if constexpr (many_v<FB>) {
		const int q = blockIdx.y;
		n = fb.src_len[q];
		if ((long)blockIdx.x * STREAM_TILE >= n)                  // (uniform: a tile past this recording's end)
			return;
		samples = (const char *)fb.samples + (size_t)q * fb.frame_stride_bytes;
		fn += fb.tile0[q];
		carry += fb.tile0[q];
		edges += (size_t)q * cap;
		if constexpr (GIVEN)
			given += fb.given0[q];
	}
	if constexpr (bank_v<FB>) {                                   // channel blockIdx.y: its window, its tiles of this push, its places
		static_assert(!GIVEN, "a bank scans windows of sample streams");
		const int q = blockIdx.y;
		if ((long long)blockIdx.x >= fb.tile_at[q + 1] - fb.tile_at[q])   // (uniform: this channel brings fewer tiles)
			return;
		n = (long)fb.len[q];
		samples = batch_base(fb, q);
		tile0 = fb.tile0[q];
		fn += fb.tile_at[q];
		carry += fb.tile_at[q];
		edges += (size_t)q * cap;
	}
	typedef RateCfg<RATE> RC;
	constexpr int HS = RC::HS, GL = RC::GL, ML = RC::MATCH_LEN, MD = RC::MATCH_DEL;
	constexpr int D = RC::BUFFER_LEN - 1 - (RC::SEARCH_POS + HS);   // P at time t: its newest pair is (t - D, t - D + HS)
	constexpr int L = STREAM_TILE + ML - 1, PM = (L + 255) / 256;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const long long T0 = ((long long)blockIdx.x + (bank_v<FB> ? tile0 : 0)) * STREAM_TILE;
	const float lo = (float)(0.17 * ML), hi = (float)(0.19 * ML);   // decode.cc:76
	__shared__ TrigShared tsh;
	float v[SPT];
	if constexpr (GIVEN) {
		for (int j = 0; j < SPT; ++j) {
			const long long t = T0 + tid * SPT + j;
			v[j] = t < n ? given[t] : 0.f;
		}
	} else {
		// decode.cc:86-90 at the times tm0 .. T0 + STREAM_TILE - 1: P and R as window sums in double - direct sums at tm0 - 1, then the
		// (in - out) differences, prefix-summed over the tile - and m = |P|^2 / R^2 in the reference's fp32 expression; timing = the
		// sum of the last ML values of m in double, rounded once
		__shared__ double Sd[L];
		__shared__ double red[3][4];
		__shared__ double3 sc3[256];
		const SampleSrc src{ samples, fb.fmt, fb.channels, n, nullptr };
		const long long tm0 = T0 - (ML - 1);
		double p0r = 0.0, p0i = 0.0, r0 = 0.0;
		{
			const long long a = tm0 - 1 - D;
			for (int k = tid; k < HS; k += 256) {
				const cf x = src.at(a - k), y = src.at(a - k + HS);
				p0r += (double)x.re * y.re + (double)x.im * y.im;
				p0i += (double)x.im * y.re - (double)x.re * y.im;
			}
			for (int k = tid; k < 2 * HS; k += 256) {
				const cf x = src.at(a + HS - k);
				r0 += (double)x.re * x.re + (double)x.im * x.im;
			}
			p0r = wave_sum_d(p0r);
			p0i = wave_sum_d(p0i);
			r0 = wave_sum_d(r0);
			if (lane == 0) {
				red[0][wave] = p0r;
				red[1][wave] = p0i;
				red[2][wave] = r0;
			}
			__syncthreads();
			p0r = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
			p0i = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
			r0 = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
		}
		double dr[PM], di[PM], dp[PM];
		for (int e = 0; e < PM; ++e) {
			const int idx = tid * PM + e;
			double pr = 0.0, pi = 0.0, pp = 0.0;
			if (idx < L) {
				const long long a = tm0 + idx - D;
				const cf zA = src.at(a - HS), zB = src.at(a), zC = src.at(a + HS);
				const double inr = (double)zB.re * zC.re + (double)zB.im * zC.im;
				const double ini = (double)zB.im * zC.re - (double)zB.re * zC.im;
				const double outr = (double)zA.re * zB.re + (double)zA.im * zB.im;
				const double outi = (double)zA.im * zB.re - (double)zA.re * zB.im;
				const double pin = (double)zC.re * zC.re + (double)zC.im * zC.im;
				const double pout = (double)zA.re * zA.re + (double)zA.im * zA.im;
				pr = inr - outr;
				pi = ini - outi;
				pp = pin - pout;
			}
			dr[e] = (e ? dr[e - 1] : 0.0) + pr;
			di[e] = (e ? di[e - 1] : 0.0) + pi;
			dp[e] = (e ? dp[e - 1] : 0.0) + pp;
		}
		block_scan_incl<256>(make_double3(dr[PM - 1], di[PM - 1], dp[PM - 1]), sc3, tid,
			[](double3 l, double3 r) { return make_double3(l.x + r.x, l.y + r.y, l.z + r.z); });
		const double3 o = tid ? sc3[tid - 1] : make_double3(0.0, 0.0, 0.0);
		__syncthreads();
		const float min_R = 0.0001f * HS;                          // decode.cc:88
		double cm = 0.0;
		for (int e = 0; e < PM; ++e) {
			const float Pre = (float)((p0r + o.x) + dr[e]), Pim = (float)((p0i + o.y) + di[e]);
			float R = 0.5f * (float)((r0 + o.z) + dp[e]);
			R = fmaxf(R, min_R);
			const float mf = __fdiv_rn(__fadd_rn(__fmul_rn(Pre, Pre), __fmul_rn(Pim, Pim)), __fmul_rn(R, R));
			cm += tid * PM + e < L ? (double)mf : 0.0;
			dr[e] = cm;
		}
		block_scan_incl<256>(make_double3(cm, 0.0, 0.0), sc3, tid,
			[](double3 l, double3 r) { return make_double3(l.x + r.x, 0.0, 0.0); });
		const double om = tid ? sc3[tid - 1].x : 0.0;
		for (int e = 0; e < PM; ++e)
			if (tid * PM + e < L)
				Sd[tid * PM + e] = om + dr[e];
		__syncthreads();
		for (int j = 0; j < SPT; ++j) {
			const int idx = ML - 1 + tid * SPT + j;                 // t - tm0
			v[j] = (float)(Sd[idx] - (idx >= ML ? Sd[idx - ML] : 0.0));
		}
	}
	int cls[SPT];
	const long long t0 = T0 + tid * SPT;
	for (int j = 0; j < SPT; ++j)
		cls[j] = t0 + j >= n ? 0 : v[j] > hi ? 1 : v[j] < lo ? -1 : 0;
	int s_thr, s_out;
	Seg seg_thr, seg_out;
	long long before, n_out;
	if constexpr (!EMIT) {
		StreamFn f;
		for (int s = 0; s < 2; ++s) {
			tile_trigger(tsh, cls, v, t0, tid, s, -INFINITY, -1, s_thr, seg_thr, before, s_out, seg_out, n_out);
			f.s_out[s] = s_out;
			f.has[s] = n_out > 0;
			f.n[s] = n_out;
			f.m[s] = seg_out.m;
			f.i[s] = seg_out.i;
		}
		if (tid == 0)
			fn[blockIdx.x] = f;
	} else {
		const StreamCarry c = carry[blockIdx.x];
		tile_trigger(tsh, cls, v, t0, tid, c.s, c.m, c.i, s_thr, seg_thr, before, s_out, seg_out, n_out);
		int s = s_thr;
		float m = seg_thr.m;
		long long im = seg_thr.i, pos = c.count + before;
		for (int j = 0; j < SPT; ++j) {
			const long long t = t0 + j;
			if (cls[j] < 0 && s == 1) {                               // decode.cc:103-116
				comb(m, im, v[j], t);
				if (pos < cap) {
					StreamEdge e;
					e.g = t;
					e.t_max = im;
					const long long age = MD + (t - im);
					e.index_max = (int)(age < HS + GL + MD ? age : HS + GL + MD);
					e.accept = 0;
					e.symbol_pos = 0;
					e.cfo_rad = 0.f;
					edges[pos] = e;
				}
				++pos;
				m = -INFINITY;
				im = -1;
			} else {
				comb(m, im, v[j], t);
			}
			if (cls[j])
				s = cls[j] > 0;
		}
	}
}

// the per-tile functions composed (l first, then r)
__device__ __forceinline__ StreamFn fn_then(const StreamFn &l, const StreamFn &r)
{
	StreamFn o;
	for (int s = 0; s < 2; ++s) {
		const int q = l.s_out[s];
		o.s_out[s] = r.s_out[q];
		o.has[s] = l.has[s] | r.has[q];
		o.n[s] = l.n[s] + r.n[q];
		if (r.has[q]) {
			o.m[s] = r.m[q];
			o.i[s] = r.i[q];
		} else {
			o.m[s] = l.m[s];
			o.i[s] = l.i[s];
			comb(o.m[s], o.i[s], r.m[q], r.i[q]);
		}
	}
	return o;
}
__device__ __forceinline__ StreamCarry fn_apply(const StreamFn &f, StreamCarry c)
{
	const int s = c.s;
	StreamCarry o;
	o.s = f.s_out[s];
	o.count = c.count + f.n[s];
	if (f.has[s]) {
		o.m = f.m[s];
		o.i = f.i[s];
	} else {
		o.m = c.m;
		o.i = c.i;
		comb(o.m, o.i, f.m[s], f.i[s]);
	}
	return o;
}

// WIN (a live channel): the scan starts from the carry the previous push left (*c_in, its edge count taken as 0) and leaves *c_out
// for the next
template <bool WIN>
__device__ __forceinline__ void fn_scan_wg(const StreamFn *__restrict__ fn, long ntiles, StreamCarry *__restrict__ carry, long long *__restrict__ counts,
	const StreamCarry *__restrict__ c_in, StreamCarry *__restrict__ c_out)
{
	const int tid = threadIdx.x;
	__shared__ StreamFn sh[1024];
	const long per = (ntiles + 1023) / 1024, k0 = (long)tid * per, k1 = k0 + per < ntiles ? k0 + per : ntiles;
	StreamFn f;
	for (int s = 0; s < 2; ++s) {
		f.s_out[s] = s;
		f.has[s] = 0;
		f.n[s] = 0;
		f.m[s] = -INFINITY;
		f.i[s] = -1;
	}
	for (long k = k0; k < k1; ++k)
		f = fn_then(f, fn[k]);
	block_scan_incl<1024>(f, sh, tid, fn_then);
	StreamCarry c{ 0, -INFINITY, -1, 0 };                     // the stream starts with the trigger off (decode.cc:68-74)
	if constexpr (WIN) {
		c = *c_in;
		c.count = 0;
	}
	if (tid)
		c = fn_apply(sh[tid - 1], c);
	for (long k = k0; k < k1; ++k) {
		carry[k] = c;
		c = fn_apply(fn[k], c);
	}
	if (k0 < ntiles && k1 == ntiles) {
		counts[0] = c.count;
		if constexpr (WIN)
			*c_out = c;
	}
}
// The segmented scan: one workgroup per recording composes that recording's tiles alone, from the initial carry (trigger off, no
// maximum, no edges) - the reset at a recording's start is that nothing of its neighbour is ever composed with it.
// counts: [recordings][2], cleared by the caller before the scan (a recording without tiles writes nothing)
__global__ __launch_bounds__(1024) void k_streams_fn_scan(const StreamFn *__restrict__ fn, const long long *__restrict__ tile0, StreamCarry *__restrict__ carry,
	long long *__restrict__ counts)
{
	const long long t0 = tile0[blockIdx.x];
	fn_scan_wg<false>(fn + t0, (long)(tile0[blockIdx.x + 1] - t0), carry + t0, counts + 2 * (size_t)blockIdx.x, nullptr, nullptr);
}

// The segmented windowed scan: one workgroup per live channel composes the tiles that channel brings in this push, from the carry
// that channel's last push left, and leaves the carry for its next one.  A channel without tiles keeps its carry.
// counts: [channels][2], cleared by the caller
__global__ __launch_bounds__(1024) void k_bank_fn_scan(const StreamFn *__restrict__ fn, const long long *__restrict__ tile_at, StreamCarry *__restrict__ carry,
	long long *__restrict__ counts, const StreamCarry *__restrict__ c_in, StreamCarry *__restrict__ c_out)
{
	const long long t0 = tile_at[blockIdx.x];
	const long nt = (long)(tile_at[blockIdx.x + 1] - t0);
	if (nt == 0) {                                                // (uniform)
		if (threadIdx.x == 0)
			c_out[blockIdx.x] = c_in[blockIdx.x];
		return;
	}
	fn_scan_wg<true>(fn + t0, nt, carry + t0, counts + 2 * (size_t)blockIdx.x, c_in + blockIdx.x, c_out + blockIdx.x);
}

void launch_streams_scan(hipStream_t s, int rate, int n_src, long max_len, SourceBatch fb, const float *given, StreamFn *fn, StreamCarry *carry,
	StreamEdge *edges, long cap, long long *counts)
{
	const dim3 grid((unsigned)((max_len + STREAM_TILE - 1) / STREAM_TILE), (unsigned)n_src);
	if (given) {
		RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, true, false, SourceBatch>), grid, dim3(256), 0, s, fb, given, 0L, fn, carry, edges, cap));
	} else {
		RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, false, false, SourceBatch>), grid, dim3(256), 0, s, fb, given, 0L, fn, carry, edges, cap));
	}
	hipLaunchKernelGGL(k_streams_fn_scan, dim3((unsigned)n_src), dim3(1024), 0, s, fn, fb.tile0, carry, counts);
	if (given) {
		RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, true, true, SourceBatch>), grid, dim3(256), 0, s, fb, given, 0L, fn, carry, edges, cap));
	} else {
		RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, false, true, SourceBatch>), grid, dim3(256), 0, s, fb, given, 0L, fn, carry, edges, cap));
	}
}

void launch_bank_scan(hipStream_t s, int rate, int n_ch, long max_tiles, WindowBatch fb, StreamFn *fn, StreamCarry *carry, const StreamCarry *c_in,
	StreamCarry *c_out, StreamEdge *edges, long cap, long long *counts)
{
	const dim3 grid((unsigned)max_tiles, (unsigned)n_ch);
	RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, false, false, WindowBatch>), grid, dim3(256), 0, s, fb, nullptr, 0L, fn, carry, edges, cap));
	hipLaunchKernelGGL(k_bank_fn_scan, dim3((unsigned)n_ch), dim3(1024), 0, s, fn, fb.tile_at, carry, counts, c_in, c_out);
	RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_tile<RATE, false, true, WindowBatch>), grid, dim3(256), 0, s, fb, nullptr, 0L, fn, carry, edges, cap));
}

// ---------------------------------------------------------------- accept, records
constexpr int ACCEPT_GRID = 2048;
// FB = SourceBatch: the edges of recording blockIdx.y (edges: [recordings][cap], counts: [recordings][2]), read from its base with its length
// FB = WindowBatch: the edges of the live channel blockIdx.y, of whose stream only the positions from fb.lo[q] on are in memory.  The
// host has checked that no edge of this push reads below it (api_bank.cpp); an edge that would is left rejected and reported in
// fb.below[q]
template <int RATE, class FB>
__global__ __launch_bounds__(256) void k_stream_accept(FB fb, const cf *__restrict__ tw, const cf *__restrict__ kern,
	StreamEdge *__restrict__ edges, long cap, long long *__restrict__ counts)
{
	static_assert(many_v<FB> || bank_v<FB>, "recordings or live channels");
	const void *samples = fb.samples;
	long n_src = fb.samples_per_frame;
	long long win_lo = 0;
	if constexpr (many_v<FB>) {
		const int q = blockIdx.y;
		samples = (const char *)fb.samples + (size_t)q * fb.frame_stride_bytes;
		n_src = fb.src_len[q];
		edges += (size_t)q * cap;
		counts += 2 * (size_t)q;
	}
	if constexpr (bank_v<FB>) {                                   // the edges of the live channel blockIdx.y, read through its window
		const int q = blockIdx.y;
		samples = batch_base(fb, q);
		n_src = (long)fb.len[q];
		edges += (size_t)q * cap;
		counts += 2 * (size_t)q;
		win_lo = fb.lo[q];
	}
	typedef RateCfg<RATE> RC;
	constexpr int BUFFER_LEN = RC::BUFFER_LEN, SEARCH_POS = RC::SEARCH_POS, HALF_LEN = RC::HS, MATCH_DEL = RC::MATCH_DEL, NT = 256;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const long long ne = counts[0] < cap ? counts[0] : cap;
	const SampleSrc src{ samples, fb.fmt, fb.channels, n_src, nullptr };
	__shared__ cf buf[HALF_LEN], xr[HALF_LEN];
	__shared__ cf rot[(HALF_LEN + NT - 1) / NT];
	__shared__ float red_p[4];
	__shared__ int red_i[4];
	__shared__ float phase_sh;
	for (long long e = blockIdx.x; e < ne; e += gridDim.x) {
		__syncthreads();
		StreamEdge ed = edges[e];
		if constexpr (bank_v<FB>) {
			// the lowest positions direct_P and sc_accept_wg read for this edge
			const long long lo_p = ed.t_max - MATCH_DEL - (BUFFER_LEN - 1 - (SEARCH_POS + HALF_LEN)) - (HALF_LEN - 1);
			const long long lo_w = ed.g - (BUFFER_LEN - 1) + (SEARCH_POS - ed.index_max) + HALF_LEN;
			if (win_lo > 0 && (lo_p < win_lo || lo_w < win_lo)) {     // (uniform)
				if (tid == 0)
					fb.below[blockIdx.y] = 1;
				continue;
			}
		}
		if (wave == 0) {                                          // decode.cc:91: arg(P) delayed by match_del (k_sync: direct_P)
			float phase = 0.f;
			const long long tp = ed.t_max - MATCH_DEL;
			if (tp >= 0) {
				double pr, pi;
				direct_P<RATE>(src, (long)tp, lane, pr, pi);
				phase = atan2f((float)pi, (float)pr);
			}
			if (lane == 0)
				phase_sh = phase;
		}
		__syncthreads();
		const float phase_max = phase_sh;
		const float frac_cfo = phase_max / (float)HALF_LEN;       // decode.cc:110
		int symbol_pos = SEARCH_POS - ed.index_max;               // decode.cc:114
		const long base = (long)ed.g - (BUFFER_LEN - 1);
		int shift, pos_err;
		const bool accept = sc_accept_wg<RATE>(buf, xr, rot, red_p, red_i, src, tw, kern, base, symbol_pos, frac_cfo, tid, lane, wave, shift, pos_err);
		if (tid == 0) {
			ed.accept = accept ? 1 : 0;
			if (accept) {
				symbol_pos -= pos_err;
				float cfo_rad = (float)shift * (TWO_PI_F / (float)HALF_LEN) - frac_cfo;   // decode.cc:148
				if (cfo_rad >= PI_F)
					cfo_rad -= TWO_PI_F;
				ed.symbol_pos = symbol_pos;
				ed.cfo_rad = cfo_rad;
			}
			edges[e] = ed;
		}
	}
}

void launch_streams_accept(hipStream_t s, int rate, int n_src, SourceBatch fb, Tables tb, StreamEdge *edges, long cap, long long *counts)
{
	// (workgroups per recording: ACCEPT_GRID shared out, every recording's edges strided over its own)
	long per = ACCEPT_GRID / n_src < cap ? ACCEPT_GRID / n_src : cap;
	per = per > 0 ? per : 1;
	RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_accept<RATE, SourceBatch>), dim3((unsigned)per, (unsigned)n_src), dim3(256), 0, s, fb, tb.tw_sym, tb.sc_kern,
		edges, cap, counts));
}
void launch_bank_accept(hipStream_t s, int rate, int n_ch, WindowBatch fb, Tables tb, StreamEdge *edges, long cap, long long *counts)
{
	long per = ACCEPT_GRID / n_ch < cap ? ACCEPT_GRID / n_ch : cap;
	per = per > 0 ? per : 1;
	RX_RATE_SWITCH(rate, hipLaunchKernelGGL((k_stream_accept<RATE, WindowBatch>), dim3((unsigned)per, (unsigned)n_ch), dim3(256), 0, s, fb, tb.tw_sym, tb.sc_kern,
		edges, cap, counts));
}

// rec_src (nullable) / src: the recording (or live channel) every record written reads
__device__ __forceinline__ void stream_records_wg(int buffer_len, const StreamEdge *__restrict__ edges, long cap, long long *__restrict__ counts,
	SyncState *__restrict__ rec, long max_rec, long long rec_base, long long rej_base, int *__restrict__ rec_src, int src)
{
	const int tid = threadIdx.x;
	__shared__ long long sh[1024];
	const long long ne = counts[0] < cap ? counts[0] : cap;
	long long base = 0;
	for (long long e0 = 0; e0 < ne; e0 += 1024) {
		const long long e = e0 + tid;
		const int acc = e < ne ? edges[e].accept : 0;
		block_scan_incl<1024>((long long)acc, sh, tid, add_ll);
		const long long k = base + (tid ? sh[tid - 1] : 0);
		const long long total = sh[1023];
		__syncthreads();
		if (acc && k < max_rec) {
			const StreamEdge ed = edges[e];
			SyncState st;                                         // what k_header finds after an accepted round with skip_left = 0
			st.t_next = (long)ed.g + 1;
			st.sc_start = (long)ed.g - (buffer_len - 1) + ed.symbol_pos;
			st.active = 1;
			st.found = 1;
			st.symbol_pos = ed.symbol_pos;
			st.cfo_rad = ed.cfo_rad;
			st.rejects = (int)(rej_base + (e - k));               // the edges before it that decode.cc:140-145 rejected (rej_base: in earlier pushes of a live channel)
			st.skip_left = 0;
			st.status = 1;
			st.oper_mode = 0;
			st.call_sign = 0;
			st.hdr_rounds = (int)(rec_base + k);
			st.okay = 0;
			st.pend_g = 0;
			st.pend_index_max = 0;
			st.pend_phase = 0.f;
			st.pending = 0;
			rec[k] = st;
			if (rec_src)
				rec_src[k] = src;
		}
		base += total;
	}
	if (tid == 0)
		counts[1] = base;
}

// The recordings' accepted preambles counted (counts[q][1]), ...
__global__ __launch_bounds__(1024) void k_streams_count(const StreamEdge *__restrict__ edges, long cap, long long *__restrict__ counts)
{
	const int tid = threadIdx.x, q = blockIdx.x;
	__shared__ long long sh[1024];
	const long long ne = counts[2 * (size_t)q] < cap ? counts[2 * (size_t)q] : cap;
	long long acc = 0;
	for (long long e = tid; e < ne; e += 1024)
		acc += edges[(size_t)q * cap + e].accept;
	block_scan_incl<1024>(acc, sh, tid, add_ll);
	if (tid == 0)
		counts[2 * (size_t)q + 1] = sh[1023];
}
// ... the packed order: first[q] = the records of the recordings before q, each min(accepted, max_per_src) (one workgroup,
// a stretch of recordings per thread), first[n_src] = all of them ...
__global__ __launch_bounds__(1024) void k_streams_first(int n_src, const long long *__restrict__ counts, long long max_per_src, long long *__restrict__ first)
{
	const int tid = threadIdx.x;
	__shared__ long long sh[1024];
	const int per = (n_src + 1023) / 1024, q0 = tid * per, q1 = q0 + per < n_src ? q0 + per : n_src;
	long long mine = 0;
	for (int q = q0; q < q1; ++q)
		mine += counts[2 * (size_t)q + 1] < max_per_src ? counts[2 * (size_t)q + 1] : max_per_src;
	block_scan_incl<1024>(mine, sh, tid, add_ll);
	long long at = tid ? sh[tid - 1] : 0;
	for (int q = q0; q < q1; ++q) {
		first[q] = at;
		at += counts[2 * (size_t)q + 1] < max_per_src ? counts[2 * (size_t)q + 1] : max_per_src;
	}
	if (tid == 1023)
		first[n_src] = sh[1023];
}
// ... and every recording's records at its place in it (record indices and cumulative rejects count from the recording's own
// start), with the recording each one reads
__global__ __launch_bounds__(1024) void k_streams_records(int buffer_len, const StreamEdge *__restrict__ edges, long cap, long long *__restrict__ counts,
	const long long *__restrict__ first, SyncState *__restrict__ rec, int *__restrict__ rec_src, long long max_per_src, long long max_rec)
{
	const int q = blockIdx.x;
	const long long at = first[q];
	long long room = max_rec > at ? max_rec - at : 0;             // only the first max_rec of the packed order are written
	room = room < max_per_src ? room : max_per_src;
	stream_records_wg(buffer_len, edges + (size_t)q * cap, cap, counts + 2 * (size_t)q, rec + at, (long)room, 0, 0, rec_src + at, q);
}

// Many live channels: as k_streams_records, but record indices and rejects go on from what the channel's earlier pushes counted
__global__ __launch_bounds__(1024) void k_bank_records(int buffer_len, const StreamEdge *__restrict__ edges, long cap, long long *__restrict__ counts,
	const long long *__restrict__ first, SyncState *__restrict__ rec, int *__restrict__ rec_src, const long long *__restrict__ rec_base,
	const long long *__restrict__ rej_base, long long max_rec)
{
	const int q = blockIdx.x;
	const long long at = first[q];
	const long long room = max_rec > at ? max_rec - at : 0;       // only the first max_rec of the packed order are written
	stream_records_wg(buffer_len, edges + (size_t)q * cap, cap, counts + 2 * (size_t)q, rec + at, (long)room, rec_base[q], rej_base[q], rec_src + at, q);
}

void launch_streams_records(hipStream_t s, int rate, int n_src, const StreamEdge *edges, long cap, long long *counts, long long *first,
	SyncState *rec, int *rec_src, long long max_per_src, long long max_rec)
{
	int buffer_len = 0;
	RX_RATE_SWITCH(rate, buffer_len = RateCfg<RATE>::BUFFER_LEN);
	hipLaunchKernelGGL(k_streams_count, dim3((unsigned)n_src), dim3(1024), 0, s, edges, cap, counts);
	hipLaunchKernelGGL(k_streams_first, dim3(1), dim3(1024), 0, s, n_src, counts, max_per_src, first);
	hipLaunchKernelGGL(k_streams_records, dim3((unsigned)n_src), dim3(1024), 0, s, buffer_len, edges, cap, counts, first, rec, rec_src, max_per_src, max_rec);
}

void launch_bank_records(hipStream_t s, int rate, int n_ch, const StreamEdge *edges, long cap, long long *counts, long long *first, SyncState *rec,
	int *rec_src, const long long *rec_base, const long long *rej_base, long long max_rec)
{
	int buffer_len = 0;
	RX_RATE_SWITCH(rate, buffer_len = RateCfg<RATE>::BUFFER_LEN);
	hipLaunchKernelGGL(k_streams_count, dim3((unsigned)n_ch), dim3(1024), 0, s, edges, cap, counts);
	hipLaunchKernelGGL(k_streams_first, dim3(1), dim3(1024), 0, s, n_ch, counts, (long long)1 << 62, first);
	hipLaunchKernelGGL(k_bank_records, dim3((unsigned)n_ch), dim3(1024), 0, s, buffer_len, edges, cap, counts, first, rec, rec_src, rec_base, rej_base, max_rec);
}

// ---------------------------------------------------------------- the window move / the new samples of every channel
// Range blockIdx.z * plane_stride + blockIdx.y (the planes: raw samples, analytic signal, DC states), given by address: whole waves
// on 16-byte pieces from the first 16-byte boundary of the destination on (the source lies the same modulo 16), the bytes before it
// and behind the last whole piece one by one.  Plain vector loads and stores.
__global__ __launch_bounds__(256) void k_bank_copy(const long long *__restrict__ src, const long long *__restrict__ dst, const long long *__restrict__ bytes,
	size_t plane_stride)
{
	const size_t q = (size_t)blockIdx.z * plane_stride + blockIdx.y;
	const long long nb = bytes[q];
	if (nb <= 0)
		return;
	const char *__restrict__ sp = (const char *)(uintptr_t)src[q];
	char *__restrict__ dp = (char *)(uintptr_t)dst[q];
	long long head = (long long)((16 - ((size_t)dp & 15)) & 15);
	head = head < nb ? head : nb;
	const long long pieces = (nb - head) / 16, tail0 = head + pieces * 16;
	const long long t = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
	const uint4 *s4 = (const uint4 *)(sp + head);
	uint4 *d4 = (uint4 *)(dp + head);
	for (long long i = t; i < pieces; i += step)
		d4[i] = s4[i];
	if (t < head)
		dp[t] = sp[t];
	if (t < nb - tail0)
		dp[tail0 + t] = sp[tail0 + t];
}
void launch_bank_copy(hipStream_t s, int n_ch, int planes, size_t plane_stride, long long max_bytes, const long long *src, const long long *dst,
	const long long *bytes)
{
	// (16 pieces per thread where a range is long; never more blocks than the longest range has use for)
	long long bx = (max_bytes / 16 + 256 * 16 - 1) / (256 * 16);
	bx = bx < 1 ? 1 : bx > 4096 ? 4096 : bx;
	hipLaunchKernelGGL(k_bank_copy, dim3((unsigned)bx, (unsigned)n_ch, (unsigned)planes), dim3(256), 0, s, src, dst, bytes, plane_stride);
}

}  // namespace rx
