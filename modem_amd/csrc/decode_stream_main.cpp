// decode_stream_main.cpp -- `decode_stream OUTDIR INPUT`: every frame of a recording in one call (ofdmrx_decode_stream).
// OUTDIR/<k>.dat holds the 5380 bytes `decode OUT INPUT k` writes (descrambled; zeros for a failed frame), for every preamble k
// the SKIP loop of decode.cc:390-448 would count; one summary line per record on stderr.  Exit status 0 like `decode`
// (decode.cc:619), 1 on argument, WAV or library errors.
#include "wav_read.h"
#include <cstdlib>
#include <string>

int main(int argc, char **argv)
{
	if (argc != 3) {
		std::fprintf(stderr, "usage: %s OUTDIR INPUT\n", argv[0]);
		return 1;
	}
	const std::string outdir = argv[1];
	const char *input_name = argv[2];
	if (!std::strcmp(input_name, "-"))
		input_name = "/dev/stdin";
	Wav w;
	if (!read_wav(input_name, w) || w.frames == 0) {
		std::fprintf(stderr, "Couldn't open file \"%s\" for reading.\n", input_name);
		return 1;
	}
	if (w.channels < 1 || w.channels > 2) {
		std::fprintf(stderr, "Only real or analytic signal (one or two channels) supported.\n");
		return 1;
	}
	if (w.rate != 8000 && w.rate != 16000 && w.rate != 44100 && w.rate != 48000) {   // decode.cc:590-605
		std::fprintf(stderr, "Unsupported sample rate.\n");
		return 1;
	}
	if (ofdmrx_abi_version() != OFDMRX_ABI_VERSION || ofdmrx_abi_minor() < 7) {
		std::fprintf(stderr, "libofdmrx: ABI %d.%d, this program needs %d.7\n", ofdmrx_abi_version(), ofdmrx_abi_minor(), OFDMRX_ABI_VERSION);
		return 1;
	}
	ofdmrx_config cfg{};
	cfg.abi_version = OFDMRX_ABI_VERSION;
	cfg.sample_rate = w.rate;
	cfg.list_size = 8;
	cfg.device = 0;
	cfg.chunk_frames = 64;
	cfg.descramble = 1;
	ofdmrx_handle *h = nullptr;
	int r = ofdmrx_create(&cfg, &h);
	if (r) {
		std::fprintf(stderr, "ofdmrx_create: %s\n", ofdmrx_strerror(r));
		return 1;
	}
	size_t cap = 64, n_pre = 0;
	std::vector<uint8_t> out;
	std::vector<ofdmrx_frame_result> res;
	for (;;) {                                                    // a second call only when the recording holds more than the first guess
		out.assign(cap * OFDMRX_PAYLOAD_BYTES, 0);
		res.assign(cap, ofdmrx_frame_result{});
		r = ofdmrx_decode_stream(h, w.pcm.data(), w.fmt, w.channels, w.frames, cap, out.data(), res.data(), &n_pre);
		if (r) {
			std::fprintf(stderr, "ofdmrx_decode_stream: %s\n", ofdmrx_strerror(r));
			ofdmrx_destroy(h);
			return 1;
		}
		if (n_pre <= cap)
			break;
		cap = n_pre;
	}
	ofdmrx_destroy(h);
	static const char *names[] = { "ok", "no sync", "OSD error", "header CRC error", "mode unsupported", "call sign unsupported",
		"payload decoding error" };
	for (size_t k = 0; k < n_pre; ++k) {
		const ofdmrx_frame_result &q = res[k];
		char cs[10];
		unsigned long long v = q.call_sign;
		for (int i = 8; i >= 0; --i, v /= 37)                     // base37_decoder, decode.cc:155-159
			cs[i] = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[v % 37];
		cs[9] = 0;
		std::fprintf(stderr, "%zu: sample %lld mode %d call sign %s %s bit flips %d\n", k, (long long)q.sc_start, q.oper_mode, cs,
			q.status >= 0 && q.status <= 6 ? names[q.status] : "?", q.bit_flips);
		const std::string name = outdir + "/" + std::to_string(k) + ".dat";
		FILE *f = std::fopen(name.c_str(), "wb");
		if (!f) {
			std::fprintf(stderr, "Couldn't open file \"%s\" for writing.\n", name.c_str());
			return 1;
		}
		std::fwrite(out.data() + k * OFDMRX_PAYLOAD_BYTES, 1, OFDMRX_PAYLOAD_BYTES, f);
		std::fclose(f);
	}
	return 0;
}
