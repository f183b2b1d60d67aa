// synthesize_main.cpp -- `synthesize OUT.wav INTERP CENTRE_HZ:START:GAIN_DB:IN.wav [...]`: mixes narrowband recordings into one
// wideband I/Q capture (ofdmrx_util_synthesize).  Every IN.wav is an analytic signal (2 channels) of 8 or 16
// bits at one common supported rate; it is placed at CENTRE_HZ, START wideband samples into the capture, at GAIN_DB.  OUT.wav has 2
// channels of 16 bits at INTERP x that rate and is as long as the last channel's support: what `decode_stream --wideband INTERP
// c1,c2,.. OUTROOT OUT.wav` reads.  INTERP may be a ratio P/Q - it is one when it holds a '/' (Q <= 16,
// 2 <= P / Q <= 32; ofdmrx_util_synthesize_ratio): OUT.wav is then at that rate x P / Q, which must be an integer.
// `synthesize --grid OUT.wav INTERP SLOT:START:GAIN_DB:IN.wav [...]`: the same through the grid synthesizer (DESIGN.md section 4.20,
// ofdmrx_util_synthesize_grid): INTERP a power of two 2 .. 512, every IN.wav in a slot of its own, SLOT = -INTERP .. INTERP - 1 with
// its centre at SLOT x rate / 2, START a multiple of INTERP: what `decode_stream --grid INTERP SLOTS OUTROOT OUT.wav` reads.
// `synthesize --grid-ratio OUT.wav P/Q SLOT:START:GAIN_DB:IN.wav [...]`: the same at a ratio (DESIGN.md section 4.23,
// ofdmrx_util_synthesize_grid_ratio): in lowest terms Q <= 16, 2 Q <= P <= 512, P with no prime factor other than 2, 3 and 5; SLOT with
// -P <= SLOT x Q < P and given once, START a multiple of the reduced P; the rate x P / Q must be an integer: what `decode_stream --grid
// P/Q SLOTS OUTROOT OUT.wav` reads.  The spelling `--grid OUT.wav P/Q` keeps its refusal: folding the two is left to a later change.
// Exit status 0, or 1 on argument, WAV or library errors.
#include "survey_cli.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static void put16(uint8_t *p, uint16_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }

int main(int argc, char **argv)
{
	const char *program = argv[0];
	const bool grid = argc > 1 && !std::strcmp(argv[1], "--grid");
	const bool grid_ratio = argc > 1 && !std::strcmp(argv[1], "--grid-ratio");
	if (grid || grid_ratio) {
		++argv;
		--argc;
	}
	if (argc < 4) {
		std::fprintf(stderr, "usage: %s OUT.wav INTERP CENTRE_HZ:START:GAIN_DB:IN.wav [...]\n       %s --grid OUT.wav INTERP SLOT:START:GAIN_DB:IN.wav [...]\n"
			"       %s --grid-ratio OUT.wav P/Q SLOT:START:GAIN_DB:IN.wav [...]\n"
			"(--grid takes a power of two and refuses a ratio P/Q; a grid capture at a ratio is --grid-ratio)\n", program, program, program);
		return 1;
	}
	const char *output_name = argv[1];
	const Decimation interp(argv[2]);
	const size_t C = (size_t)(argc - 3);
	if (grid && interp.ratio) {
		std::fprintf(stderr, "The grid synthesizer at a ratio P/Q is not built (DESIGN.md section 4.22): a grid capture takes a power of two 2 .. 512.\n");
		return 1;
	}
	if (grid && (interp.ratio || interp.p < 2 || interp.p > 512 || (interp.p & (interp.p - 1)) || C > (size_t)(2 * interp.p))) {
		std::fprintf(stderr, "A grid capture takes an interpolation that is a power of two 2 .. 512 and 1 .. 2 INTERP channels.\n");
		return 1;
	}
	// the ratio grid: the reduced P, its range of slots
	int32_t k_first = 0;
	size_t n_all = 0;
	int red_p = interp.p;
	if (grid_ratio) {
		if (!interp.ratio || interp.p <= 0 || interp.q <= 0 || ofdmrx_util_grid_ratio_slots(interp.p, interp.q, &k_first, &n_all) || C > n_all) {
			std::fprintf(stderr, "A ratio-grid capture takes a ratio P/Q - in lowest terms Q <= 16, 2 Q <= P <= 512, P = 2^a 3^b 5^c - and at most one channel per slot.\n");
			return 1;
		}
		int a = interp.p, b = interp.q;
		while (b) {
			const int t = a % b;
			a = b;
			b = t;
		}
		red_p = interp.p / a;
	}
	if (!grid && !grid_ratio && (!interp.valid() || C > 65535)) {
		std::fprintf(stderr, "A wideband capture takes an interpolation of 2 .. 32 (a ratio P/Q: Q <= 16) and 1 .. 65535 channels.\n");
		return 1;
	}
	std::vector<int32_t> slot(C);
	std::vector<double> centre(C);
	std::vector<long long> start(C);
	std::vector<float> gain(C);
	std::vector<Wav> wavs(C);
	size_t longest = 0;
	for (size_t c = 0; c < C; ++c) {
		const char *p = argv[c + 3];
		char *e = nullptr;
		centre[c] = std::strtod(p, &e);
		bool ok = e != p && *e == ':';
		if (ok) {
			p = e + 1;
			start[c] = std::strtoll(p, &e, 10);
			ok = e != p && *e == ':' && start[c] >= 0;
		}
		double db = 0.0;
		if (ok) {
			p = e + 1;
			db = std::strtod(p, &e);
			ok = e != p && *e == ':' && e[1] && std::isfinite(db);
		}
		if (grid) {                                                   // a whole slot number on the grid, in a slot of its own; START on the grid of INTERP
			slot[c] = (int32_t)std::lrint(centre[c]);
			const bool fits = ok && centre[c] == (double)slot[c] && slot[c] >= -interp.p && slot[c] < interp.p && start[c] % interp.p == 0 &&
				std::find(slot.begin(), slot.begin() + (long)c, slot[c]) == slot.begin() + (long)c;
			if (!fits) {
				std::fprintf(stderr, "A grid channel is SLOT:START:GAIN_DB:IN.wav, SLOT = -INTERP .. INTERP - 1 and given once, START a multiple of INTERP.\n");
				return 1;
			}
		}
		if (grid_ratio && ok) {
			slot[c] = (int32_t)std::lrint(centre[c]);
			if (centre[c] != (double)slot[c] || slot[c] < k_first || slot[c] > k_first + (int32_t)n_all - 1) {
				std::fprintf(stderr, "A ratio-grid channel's slot is a whole number %d .. %d (-P <= SLOT x Q < P): %s\n", k_first, k_first + (int)n_all - 1, argv[c + 3]);
				return 1;
			}
			if (std::find(slot.begin(), slot.begin() + (long)c, slot[c]) != slot.begin() + (long)c) {
				std::fprintf(stderr, "Slot %d is given twice.\n", slot[c]);
				return 1;
			}
			if (start[c] % red_p) {
				std::fprintf(stderr, "START %lld is not a multiple of P = %d.\n", start[c], red_p);
				return 1;
			}
		}
		if (!ok) {
			std::fprintf(stderr, "A channel is CENTRE_HZ:START:GAIN_DB:IN.wav, START a count of wideband samples.\n");
			return 1;
		}
		gain[c] = (float)std::pow(10.0, db / 20.0);
		const char *input_name = e + 1;
		Wav &w = wavs[c];
		if (!read_wav(input_name, w) || w.frames == 0) {
			std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
			return 1;
		}
		if (w.channels != 2 || (w.bits != 8 && w.bits != 16)) {
			std::fprintf(stderr, "A channel is an analytic signal (two channels) of 8 or 16 bits.\n");
			return 1;
		}
		if (w.rate != wavs[0].rate) {
			std::fprintf(stderr, "The channels do not share one sample rate.\n");
			return 1;
		}
		longest = std::max(longest, w.frames);
	}
	const int rate = wavs[0].rate;
	if (rate != 8000 && rate != 16000 && rate != 44100 && rate != 48000) {
		std::fprintf(stderr, "Unsupported sample rate.\n");
		return 1;
	}
	const long long wide_num = (long long)rate * interp.p;
	if (wide_num % interp.q) {
		std::fprintf(stderr, "The capture's rate %d x %d / %d is not an integer.\n", rate, interp.p, interp.q);
		return 1;
	}
	if (ofdmrx_abi_version() != OFDMRX_ABI_VERSION || ofdmrx_abi_minor() < 9) {
		std::fprintf(stderr, "libofdmrx: ABI %d.%d, this program needs %d.9\n", ofdmrx_abi_version(), ofdmrx_abi_minor(), OFDMRX_ABI_VERSION);
		return 1;
	}
	// every row as fp32 I/Q, scaled as the decoder scales its input; the rows share the longest length, zeros behind a shorter one
	long long n_out = 0;
	std::vector<float> rows(C * longest * 2, 0.f);
	for (size_t c = 0; c < C; ++c) {
		const Wav &w = wavs[c];
		float *d = rows.data() + c * longest * 2;
		for (size_t i = 0; i < 2 * w.frames; ++i)
			d[i] = w.bits == 16 ? (float)((const int16_t *)w.pcm.data())[i] / 32767.f : (float)((int)w.pcm[i] - 128) / 127.f;
		n_out = std::max(n_out, start[c] + (((long long)w.frames - 1 + 24) * interp.p) / interp.q + 1);
		wavs[c].pcm = std::vector<uint8_t>();
	}
	const unsigned long long bytes = (unsigned long long)n_out * 4;
	if (bytes > 0xffffffffull - 36) {
		std::fprintf(stderr, "The capture does not fit a WAV file.\n");
		return 1;
	}
	ofdmrx_config cfg{};
	cfg.abi_version = OFDMRX_ABI_VERSION;
	cfg.sample_rate = rate;
	cfg.list_size = 8;
	cfg.chunk_frames = 1;
	cfg.descramble = 1;
	ofdmrx_handle *h = nullptr;
	int r = ofdmrx_create(&cfg, &h);
	if (r) {
		std::fprintf(stderr, "ofdmrx_create: %s\n", ofdmrx_strerror(r));
		return 1;
	}
	std::vector<int16_t> pcm((size_t)n_out * 2);
	void *d_in = nullptr, *d_out = nullptr;
	hipError_t e = hipMalloc(&d_in, rows.size() * sizeof(float));
	e = e == hipSuccess ? hipMalloc(&d_out, (size_t)bytes) : e;
	e = e == hipSuccess ? hipMemcpy(d_in, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice) : e;
	if (e == hipSuccess) {
		r = grid_ratio ? ofdmrx_util_synthesize_grid_ratio(h, d_in, OFDMRX_FMT_F32, longest, longest, interp.p, interp.q, slot.data(), start.data(),
			gain.data(), C, 0, (size_t)n_out, d_out, OFDMRX_FMT_S16)
			: grid ? ofdmrx_util_synthesize_grid(h, d_in, OFDMRX_FMT_F32, longest, longest, interp.p, slot.data(), start.data(), gain.data(), C, 0,
			(size_t)n_out, d_out, OFDMRX_FMT_S16)
			: interp.ratio ? ofdmrx_util_synthesize_ratio(h, d_in, OFDMRX_FMT_F32, longest, longest, interp.p, interp.q, centre.data(), start.data(),
			gain.data(), C, 0, (size_t)n_out, d_out, OFDMRX_FMT_S16)
			: ofdmrx_util_synthesize(h, d_in, OFDMRX_FMT_F32, longest, longest, interp.p, centre.data(), start.data(), gain.data(), C, 0, (size_t)n_out,
			d_out, OFDMRX_FMT_S16);
		r = r ? r : ofdmrx_synchronize(h);
		if (r)
			std::fprintf(stderr, "ofdmrx_util_synthesize: %s\n", ofdmrx_strerror(r));
		else
			e = hipMemcpy(pcm.data(), d_out, (size_t)bytes, hipMemcpyDeviceToHost);
	}
	if (e != hipSuccess)
		std::fprintf(stderr, "synthesize: %s\n", hipGetErrorString(e));
	(void)hipFree(d_in);
	(void)hipFree(d_out);
	ofdmrx_destroy(h);
	if (r || e != hipSuccess)
		return 1;
	FILE *o = std::fopen(output_name, "wb");
	if (!o) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for writing.\n", output_name);
		return 1;
	}
	uint8_t hd[44];
	const uint32_t wide = (uint32_t)(wide_num / interp.q);
	std::memcpy(hd, "RIFF", 4); put32(hd + 4, (uint32_t)(36 + bytes)); std::memcpy(hd + 8, "WAVEfmt ", 8);
	put32(hd + 16, 16); put16(hd + 20, 1); put16(hd + 22, 2); put32(hd + 24, wide);
	put32(hd + 28, wide * 4); put16(hd + 32, 4); put16(hd + 34, 16);
	std::memcpy(hd + 36, "data", 4); put32(hd + 40, (uint32_t)bytes);
	const bool wrote = std::fwrite(hd, 1, 44, o) == 44 && std::fwrite(pcm.data(), 1, (size_t)bytes, o) == (size_t)bytes;
	if (std::fclose(o) || !wrote) {
		std::fprintf(stderr, "Couldn't write file \"%s\".\n", output_name);
		return 1;
	}
	return 0;
}
