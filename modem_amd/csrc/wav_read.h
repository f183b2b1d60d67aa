// wav_read.h -- the WAV readers of the decode CLIs (decode_main.cpp, decode_stream_main.cpp): DSP::ReadWAV's contract, for a whole
// file (read_wav) or header first and then block by block as the body arrives (wav_open / wav_read_block: a pipe, a live recorder)
#pragma once
#include "../../include/ofdmrx.h"
#include <cstdio>
#include <cstring>
#include <vector>

static uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

struct Wav { int rate = 0, bits = 0, channels = 0, fmt = -1; size_t frames = 0; std::vector<uint8_t> pcm; };

// DSP::ReadWAV contract (decode.cc:576-578,590): RIFF/WAVE PCM, 8-bit unsigned, 16/24/32-bit signed LE
static bool read_wav(const char *name, Wav &w)
{
	FILE *f = std::fopen(name, "rb");
	if (!f)
		return false;
	std::vector<uint8_t> buf;
	uint8_t tmp[65536];
	size_t n;
	while ((n = std::fread(tmp, 1, sizeof(tmp), f)) > 0)
		buf.insert(buf.end(), tmp, tmp + n);
	std::fclose(f);
	if (buf.size() < 12 || std::memcmp(buf.data(), "RIFF", 4) || std::memcmp(buf.data() + 8, "WAVE", 4))
		return false;
	size_t pos = 12;
	bool have_fmt = false;
	while (pos + 8 <= buf.size()) {
		uint32_t sz = rd32(&buf[pos + 4]);
		const uint8_t *body = &buf[pos + 8];
		if (!std::memcmp(&buf[pos], "fmt ", 4) && sz >= 16) {
			w.channels = rd16(body + 2);
			w.rate = (int)rd32(body + 4);
			w.bits = rd16(body + 14);
			have_fmt = true;
		} else if (!std::memcmp(&buf[pos], "data", 4) && have_fmt) {
			size_t avail = buf.size() - (pos + 8);
			if (sz > avail)
				sz = (uint32_t)avail;
			int bytes = w.bits / 8;
			if (bytes < 1 || bytes > 4 || w.channels < 1)
				return false;
			w.frames = sz / (size_t)(bytes * w.channels);
			size_t cnt = w.frames * (size_t)w.channels;
			if (bytes == 1) {
				w.fmt = OFDMRX_FMT_U8;
				w.pcm.assign(body, body + cnt);
			} else if (bytes == 2) {
				w.fmt = OFDMRX_FMT_S16;
				w.pcm.assign(body, body + 2 * cnt);   // little endian host
			} else {
				w.fmt = OFDMRX_FMT_F32;
				w.pcm.resize(4 * cnt);
				float *d = (float *)w.pcm.data();
				float factor = (float)((1u << (w.bits - 1)) - 1);
				for (size_t i = 0; i < cnt; ++i) {
					int32_t v = 0;
					for (int b = 0; b < bytes; ++b)
						v |= (int32_t)((uint32_t)body[bytes * i + b] << (8 * b + 8 * (4 - bytes)));
					v >>= 8 * (4 - bytes);
					d[i] = (float)v / factor;
				}
			}
			return true;
		}
		pos += 8 + (size_t)sz + (sz & 1);
	}
	return false;
}

// ---- header, then blocks: nothing is read ahead of what is asked for and nothing seeks, so a pipe works
struct WavStream {
	FILE *f = nullptr;
	int rate = 0, bits = 0, channels = 0, fmt = -1;
	bool bounded = false;                                     // the data chunk states its size (else: the body runs to the end of the input)
	size_t left = 0;                                          // bytes of the data chunk not read yet, when bounded
};
static bool wav_skip(FILE *f, size_t n)
{
	uint8_t tmp[4096];
	while (n) {
		const size_t k = std::fread(tmp, 1, n < sizeof(tmp) ? n : sizeof(tmp), f);
		if (!k)
			return false;
		n -= k;
	}
	return true;
}
// the chunks up to the start of the data chunk's body (read_wav's rules for them)
static bool wav_open(const char *name, WavStream &w)
{
	w.f = std::fopen(name, "rb");
	if (!w.f)
		return false;
	uint8_t hd[12], ck[8], fm[16];
	if (std::fread(hd, 1, 12, w.f) != 12 || std::memcmp(hd, "RIFF", 4) || std::memcmp(hd + 8, "WAVE", 4))
		return false;
	bool have_fmt = false;
	while (std::fread(ck, 1, 8, w.f) == 8) {
		const uint32_t sz = rd32(ck + 4);
		if (!std::memcmp(ck, "fmt ", 4) && sz >= 16) {
			if (std::fread(fm, 1, 16, w.f) != 16 || !wav_skip(w.f, (size_t)sz - 16 + (sz & 1)))
				return false;
			w.channels = rd16(fm + 2);
			w.rate = (int)rd32(fm + 4);
			w.bits = rd16(fm + 14);
			have_fmt = true;
		} else if (!std::memcmp(ck, "data", 4) && have_fmt) {
			const int bytes = w.bits / 8;
			if (bytes < 1 || bytes > 4 || w.channels < 1)
				return false;
			w.fmt = bytes == 1 ? OFDMRX_FMT_U8 : bytes == 2 ? OFDMRX_FMT_S16 : OFDMRX_FMT_F32;
			w.bounded = sz != 0 && sz != 0xffffffffu;             // (a recorder that does not know the length writes 0 or all ones)
			w.left = sz;
			return true;
		} else if (!wav_skip(w.f, (size_t)sz + (sz & 1))) {
			return false;
		}
	}
	return false;
}
// up to `frames` more sample frames into pcm (the layout read_wav gives: 8-bit and 16-bit samples as they are, 24 / 32-bit as float);
// returns the frames read - fewer than asked for only at the end of the body
static size_t wav_read_block(WavStream &w, size_t frames, std::vector<uint8_t> &pcm)
{
	const size_t bytes = (size_t)(w.bits / 8), fb = bytes * (size_t)w.channels;
	size_t want = frames * fb;
	if (w.bounded && want > w.left)
		want = w.left;
	std::vector<uint8_t> body(want);
	const size_t got = want ? std::fread(body.data(), 1, want, w.f) : 0;
	if (w.bounded)
		w.left -= got;
	const size_t n = got / fb, cnt = n * (size_t)w.channels;
	if (bytes <= 2) {
		pcm.assign(body.begin(), body.begin() + (long)(cnt * bytes));
	} else {
		pcm.resize(4 * cnt);
		float *d = (float *)pcm.data();
		const float factor = (float)((1u << (w.bits - 1)) - 1);
		for (size_t i = 0; i < cnt; ++i) {
			int32_t v = 0;
			for (size_t b = 0; b < bytes; ++b)
				v |= (int32_t)((uint32_t)body[bytes * i + b] << (8 * b + 8 * (4 - bytes)));
			v >>= 8 * (4 - bytes);
			d[i] = (float)v / factor;
		}
	}
	return n;
}
