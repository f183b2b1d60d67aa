// api_stream.cpp -- ofdmrx_decode_stream*: every preamble of one recording in one call (revision 1.7).
//   the stream scan (k_stream.hip): [mono: the DC blocker's kept states by a scan over tiles, the analytic signal of the stream]
//   | the timing metric and the trigger as a scan over tiles | decode.cc:110-151 for every falling edge | records: the SyncState
//   of every accepted preamble, as a SKIP round with skip_left = 0 leaves it
//   one read-back of the edge / preamble counts (the call's host synchronisation)
//   the records through the chunk pipeline of the batch entries (api_pipeline.cpp: decode_records), every frame = the whole stream
#include "api_internal.h"

// fb: the whole recording as one frame (stride 0)
static int stream_args(ofdmrx_handle *h, FrameBatch fb, size_t max_frames, const void *payload, const void *results, const size_t *n_preambles)
{
	if (!h || !n_preambles || fb.samples_per_frame <= 0 || fb.samples_per_frame > 0x7fffffffL / 2)
		return OFDMRX_E_ARG;
	if (max_frames && (!payload || !results))
		return OFDMRX_E_ARG;
	return check_samples(fb.samples, fb.fmt, fb.channels);        // (like the batch entries)
}

// the scan's launches for the 2-channel view fb2 of the stream: edges, accept, records (at most max_rec)
static int enqueue_scan(ofdmrx_handle *h, FrameBatch fb2, long n, long max_rec)
{
	hipStream_t s = h->stream;
	const long ntiles = (n + STREAM_TILE - 1) / STREAM_TILE;
	const long cap = h->sx_edge_cap;
	int r = h->sx_fn.ensure((size_t)ntiles * sizeof(StreamFn));
	r = r ? r : h->sx_carry.ensure((size_t)ntiles * sizeof(StreamCarry));
	r = r ? r : h->sx_edges.ensure((size_t)cap * sizeof(StreamEdge));
	r = r ? r : h->sx_rec.ensure((size_t)std::max(1L, max_rec) * sizeof(SyncState));
	if (r)
		return r;
	launch_stream_scan(s, h->rate, fb2, nullptr, n, h->sx_fn.as<StreamFn>(), h->sx_carry.as<StreamCarry>(), h->sx_edges.as<StreamEdge>(), cap,
		h->sx_counts.as<long long>());
	launch_stream_accept(s, h->rate, fb2, h->dev, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
	launch_stream_records(s, h->rate, h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>(), h->sx_rec.as<SyncState>(), max_rec);
	HIP_OK(hipGetLastError());
	return 0;
}

// The stream scan of fb (the recording, in device memory) and the records through the pipeline.  *n_pre: accepted preambles.
// out has no attempt log: stream calls do not write it, every record is one preamble's outcome already
static int decode_stream_dev(ofdmrx_handle *h, FrameBatch fb, size_t max_frames, Outputs out, size_t *n_pre)
{
	hipStream_t s = h->stream;
	const long n = fb.samples_per_frame;
	begin_call(h);
	int r = ensure_events(h, 16);
	r = r ? r : h->sx_counts.ensure(2 * sizeof(long long));
	if (r)
		return r;
	if (h->sx_edge_cap == 0)                                      // a preamble every frame and a few noise triggers fit (else: grown below)
		h->sx_edge_cap = std::max(4096L, n / 2048);
	const size_t e0 = mark(h, s);
	FrameBatch fb2 = fb;                                          // what the scan and the pipeline read: I/Q pairs
	if (fb.channels == 1) {                                       // D1 over the whole stream, then its analytic signal read as I/Q pairs
		const long ntiles = (n + 4095) / 4096;
		const int ck_n = mono_ck_per_frame(n);
		r = h->sx_dc_end.ensure((size_t)ntiles * sizeof(double));
		r = r ? r : h->sx_dc_in.ensure((size_t)ntiles * sizeof(double));
		r = r ? r : h->sx_ck.ensure((size_t)ck_n * sizeof(double));
		r = r ? r : h->sx_z.ensure((size_t)n * sizeof(cf));
		if (r)
			return r;
		Range rg("ofdmrx:stream_front");
		launch_stream_dc(s, fb, h->host.front, h->sx_dc_end.as<double>(), h->sx_dc_in.as<double>(), h->sx_ck.as<double>());
		launch_front_end(s, h->rate, 1, fb, mono_args(h->host.front, h->sx_ck.as<double>(), ck_n), h->sx_z.as<cf>());
		fb2 = FrameBatch{ h->sx_z.p, 0, n, OFDMRX_FMT_F32, 2 };
	}
	const size_t e1 = mark(h, s);
	long long counts[2] = { 0, 0 };
	long max_rec = 0;
	for (int pass = 0; pass < 2; ++pass) {
		max_rec = (long)std::min<size_t>(max_frames, (size_t)h->sx_edge_cap);
		{
			Range rg("ofdmrx:stream_scan");
			r = enqueue_scan(h, fb2, n, max_rec);
		}
		if (r)
			return r;
		// the call's one host synchronisation: how many edges / preambles the stream holds plans the records into chunks
		HIP_OK(hipMemcpyAsync(counts, h->sx_counts.p, sizeof(counts), hipMemcpyDeviceToHost, s));
		HIP_OK(hipStreamSynchronize(s));
		if (counts[0] <= h->sx_edge_cap)
			break;
		h->sx_edge_cap = (long)counts[0];                         // more falling edges than the buffer held: once more with room for all
	}
	const size_t e2 = mark(h, s);
	h->spans.push_back({ OFDMRX_T_FRONT, e0, e1 });
	h->spans.push_back({ OFDMRX_T_SYNC, e1, e2 });
	*n_pre = (size_t)counts[1];
	const size_t n_rec = std::min<size_t>((size_t)counts[1], max_frames);
	if (n_rec == 0) {
		h->last_n = 0;
		h->last_first = 0;
		HIP_OK(hipStreamSynchronize(s));
		return finish_call(h, 0);
	}
	return decode_records(h, fb2, h->sx_rec.as<SyncState>(), n_rec, out);
}

extern "C" int ofdmrx_decode_stream_device(ofdmrx_handle *h, const void *d_samples, int fmt, int channels, size_t n_samples,
	size_t max_frames, uint8_t *d_payload_out, ofdmrx_frame_result *d_results, size_t *n_preambles)
{
	const FrameBatch fb{ d_samples, 0, (long)n_samples, fmt, channels };
	int r = stream_args(h, fb, max_frames, d_payload_out, d_results, n_preambles);
	if (r || h->busy_live())                                      // (a handle with an open feed or bank decodes nothing else)
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	return decode_stream_dev(h, fb, max_frames, Outputs{ d_payload_out, (Result *)d_results, h->esn0_user }, n_preambles);
}

extern "C" int ofdmrx_decode_stream(ofdmrx_handle *h, const void *samples, int fmt, int channels, size_t n_samples,
	size_t max_frames, uint8_t *payload_out, ofdmrx_frame_result *results, size_t *n_preambles)
{
	int r = stream_args(h, FrameBatch{ samples, 0, (long)n_samples, fmt, channels }, max_frames, payload_out, results, n_preambles);
	if (r || h->busy_live())
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	const size_t in_bytes = n_samples * sample_bytes(fmt) * (size_t)channels;
	r = h->sx_in.ensure(in_bytes);
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(h->sx_in.p, samples, in_bytes, hipMemcpyHostToDevice, h->stream));
	const FrameBatch fb{ h->sx_in.p, 0, (long)n_samples, fmt, channels };
	// outputs: device staging for as many records as the stream can hold (at most one per edge), copied out behind the call;
	// the Es/N0 rows likewise, in place of the caller's host array
	float *const rows_user = h->esn0_user;
	auto stage = [&](size_t frames) -> int {
		int rr = h->sx_pay.ensure(std::max<size_t>(1, frames) * PAYLOAD_BYTES);
		rr = rr ? rr : h->sx_res.ensure(std::max<size_t>(1, frames) * sizeof(Result));
		const size_t cap = h->sx_pay.bytes / PAYLOAD_BYTES;
		return (rr || !rows_user) ? rr : h->sx_esn0.ensure(std::max<size_t>(1, cap) * ROWS_MAX * sizeof(float));
	};
	auto staged = [&] { return Outputs{ h->sx_pay.as<uint8_t>(), h->sx_res.as<Result>(), rows_user ? h->sx_esn0.as<float>() : nullptr }; };
	r = stage(std::min<size_t>(max_frames, (size_t)std::max(4096L, (long)(n_samples / 2048))));
	if (r)
		return r;
	size_t n_pre = 0;
	// a first pass finds how many records there are
	r = decode_stream_dev(h, fb, std::min(max_frames, h->sx_pay.bytes / PAYLOAD_BYTES), staged(), &n_pre);
	if (r)
		return r;
	const size_t n_rec = std::min(n_pre, max_frames);
	if (n_rec > h->sx_pay.bytes / PAYLOAD_BYTES) {                // more records than the staging held (a stream of many short frames): again, with room
		r = stage(n_rec);
		r = r ? r : decode_stream_dev(h, fb, n_rec, staged(), &n_pre);
		if (r)
			return r;
	}
	if (n_rec) {
		HIP_OK(hipMemcpyAsync(payload_out, h->sx_pay.p, n_rec * PAYLOAD_BYTES, hipMemcpyDeviceToHost, h->stream));
		HIP_OK(hipMemcpyAsync(results, h->sx_res.p, n_rec * sizeof(Result), hipMemcpyDeviceToHost, h->stream));
		if (rows_user)
			HIP_OK(hipMemcpyAsync(rows_user, h->sx_esn0.p, n_rec * ROWS_MAX * sizeof(float), hipMemcpyDeviceToHost, h->stream));
	}
	HIP_OK(hipStreamSynchronize(h->stream));
	*n_preambles = n_pre;
	return 0;
}

extern "C" int ofdmrx_debug_stream_edges(ofdmrx_handle *h, const float *timing, size_t n, size_t max_edges,
	int64_t *t_edge, int64_t *t_max, int32_t *index_max, size_t *n_edges)
{
	if (!h || !timing || !n_edges || n == 0 || n > (size_t)0x7fffffff / 2)
		return OFDMRX_E_ARG;
	if (max_edges && (!t_edge || !t_max || !index_max))
		return OFDMRX_E_ARG;
	HIP_OK(hipSetDevice(h->cfg.device));
	hipStream_t s = h->stream;
	const long ntiles = (long)((n + STREAM_TILE - 1) / STREAM_TILE);
	const long cap = (long)std::max<size_t>(1, max_edges);
	int r = h->sx_timing.ensure(n * sizeof(float));
	r = r ? r : h->sx_fn.ensure((size_t)ntiles * sizeof(StreamFn));
	r = r ? r : h->sx_carry.ensure((size_t)ntiles * sizeof(StreamCarry));
	r = r ? r : h->sx_edges.ensure((size_t)cap * sizeof(StreamEdge));
	r = r ? r : h->sx_counts.ensure(2 * sizeof(long long));
	if (r)
		return r;
	HIP_OK(hipMemcpyAsync(h->sx_timing.p, timing, n * sizeof(float), hipMemcpyHostToDevice, s));
	launch_stream_scan(s, h->rate, FrameBatch{ nullptr, 0, (long)n, OFDMRX_FMT_F32, 2 }, h->sx_timing.as<float>(), (long)n, h->sx_fn.as<StreamFn>(),
		h->sx_carry.as<StreamCarry>(), h->sx_edges.as<StreamEdge>(), cap, h->sx_counts.as<long long>());
	HIP_OK(hipGetLastError());
	long long count = 0;
	HIP_OK(hipMemcpyAsync(&count, h->sx_counts.p, sizeof(count), hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
	const size_t w = std::min<size_t>((size_t)count, max_edges);
	if (w) {
		std::vector<StreamEdge> e(w);
		HIP_OK(hipMemcpy(e.data(), h->sx_edges.p, w * sizeof(StreamEdge), hipMemcpyDeviceToHost));
		for (size_t i = 0; i < w; ++i) {
			t_edge[i] = e[i].g;
			t_max[i] = e[i].t_max;
			index_max[i] = e[i].index_max;
		}
	}
	*n_edges = (size_t)count;
	return 0;
}
