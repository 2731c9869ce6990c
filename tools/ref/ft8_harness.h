// What tools/ref/ref_ft8_main.cpp (the reference's own statements, cut at run time by tools/make_ref_ft8_golden.py) and
// tools/ft8_host_driver.cpp (csrc/kg_ft8.h on the host) share: the scene they read, the records they write, and the independent
// double-precision DFT that stands in for kiss_fftr where a build asks for it.  Nothing here is the reference's.
//
//   <exe> scene.bin out.bin
// scene.bin: int32[8] {kind, protocol, a, b, c, d, 0, 0}
//   kind 0, LOAD:    a num_blocks, b num_candidates, c min_score; then the waterfall bytes [a][2][2][num_bins]
//   kind 1, STREAM:  a ns, b the number of callbacks, c the callback ahead of which decode_ft8_protocol is called (-1: never), d its
//                    protocol; then double times[b], int16 samples[b][a]
// out.bin: records {int32 tag, int32 bytes, payload}
//   1 SIZES  int32 block_size, nfft, num_bins, min_bin, max_blocks, num_samples, block_stride, subblock_size; float window[nfft]
//   2 EVENT  int32 cb, kind (0 SLOT_START, 1 DECODE), a, b; int64 t
//   3 SLOT   int32 cb, num_blocks, ncand, 0; float max_mag; ncand x {int16 score, time_offset, freq_offset; uint8 time_sub, freq_sub;
//            float freq_hz, time_sec, snr}; float log174[ncand][174]; the waterfall bytes [num_blocks][block_stride]
//   4 END    int32 tsync, in_pos, frame_pos, num_blocks, slot, decode_time, nfft, 0; float max_mag; float last_frame[nfft]; the
//            waterfall bytes of the slot under way
#ifndef FT8_HARNESS_H
#define FT8_HARNESS_H
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

enum { H_LOAD = 0, H_STREAM = 1 };
enum { T_SIZES = 1, T_EVENT = 2, T_SLOT = 3, T_END = 4 };
#define H_SNR_ADJ (-22.0f)

struct h_cand { int16_t score, time_offset, freq_offset; uint8_t time_sub, freq_sub; float freq_hz, time_sec, snr; };
static_assert(sizeof(h_cand) == 20, "h_cand");

struct h_scene {
    int32_t hd[8];
    std::vector<uint8_t> mag;
    std::vector<double> times;
    std::vector<int16_t> samples;
};
static inline int h_read_scene(const char *path, h_scene &s)
{
    FILE *f = fopen(path, "rb");
    if (!f || fread(s.hd, 4, 8, f) != 8) return 2;
    if (s.hd[0] == H_LOAD) {
        fseek(f, 0, SEEK_END);
        const long n = ftell(f) - 32;
        fseek(f, 32, SEEK_SET);
        s.mag.resize((size_t) n);
        if (n && fread(s.mag.data(), 1, (size_t) n, f) != (size_t) n) return 2;
    } else {
        s.times.resize((size_t) s.hd[3]);
        s.samples.resize((size_t) s.hd[3] * s.hd[2]);
        if (fread(s.times.data(), 8, s.times.size(), f) != s.times.size()) return 2;
        if (fread(s.samples.data(), 2, s.samples.size(), f) != s.samples.size()) return 2;
    }
    fclose(f);
    return 0;
}

static FILE *h_out;
static inline void h_rec(int tag, const std::vector<uint8_t> &b)
{
    const int32_t hd[2] = {tag, (int32_t) b.size()};
    fwrite(hd, 4, 2, h_out);
    if (!b.empty()) fwrite(b.data(), 1, b.size(), h_out);
}
template <typename T> static inline void h_put(std::vector<uint8_t> &b, const T *p, size_t n)
{
    const uint8_t *q = (const uint8_t *) p;
    b.insert(b.end(), q, q + sizeof(T) * n);
}
static inline void h_sizes(int block_size, int nfft, int num_bins, int min_bin, int max_blocks, int num_samples, int block_stride, int subblock_size, const float *window)
{
    std::vector<uint8_t> b;
    const int32_t v[8] = {block_size, nfft, num_bins, min_bin, max_blocks, num_samples, block_stride, subblock_size};
    h_put(b, v, 8);
    h_put(b, window, (size_t) nfft);
    h_rec(T_SIZES, b);
}
static inline void h_event(int cb, int kind, int a, int bb, int64_t t)
{
    std::vector<uint8_t> b;
    const int32_t v[4] = {cb, kind, a, bb};
    h_put(b, v, 4);
    h_put(b, &t, 1);
    h_rec(T_EVENT, b);
}
static inline void h_slot(int cb, int num_blocks, int ncand, float max_mag, const h_cand *cand, const float *log174, const uint8_t *mag, size_t nmag)
{
    std::vector<uint8_t> b;
    const int32_t v[4] = {cb, num_blocks, ncand, 0};
    h_put(b, v, 4);
    h_put(b, &max_mag, 1);
    h_put(b, cand, (size_t) ncand);
    h_put(b, log174, (size_t) ncand * 174);
    h_put(b, mag, nmag);
    h_rec(T_SLOT, b);
}
static inline void h_end(int tsync, int in_pos, int frame_pos, int num_blocks, uint32_t slot, uint32_t decode_time, int nfft, float max_mag, const float *last_frame,
                         const uint8_t *mag, size_t nmag)
{
    std::vector<uint8_t> b;
    const int32_t v[8] = {tsync, in_pos, frame_pos, num_blocks, (int32_t) slot, (int32_t) decode_time, nfft, 0};
    h_put(b, v, 8);
    h_put(b, &max_mag, 1);
    h_put(b, last_frame, (size_t) nfft);
    h_put(b, mag, nmag);
    h_rec(T_END, b);
}

// bins lo .. hi of the nfft-point DFT of a real sequence, in double, rounded to float: out[2 k], out[2 k + 1] = re, im of bin k.
// The phase table is exact to double rounding per entry (index k n mod nfft: no recurrence).
static inline void h_dft_double(int nfft, const float *in, float *out, int lo, int hi)
{
    static std::vector<double> co, si;
    if ((int) co.size() != nfft) {
        co.resize((size_t) nfft); si.resize((size_t) nfft);
        for (int i = 0; i < nfft; i++) { co[i] = cos(-2.0 * M_PI * i / nfft); si[i] = sin(-2.0 * M_PI * i / nfft); }
    }
    for (int k = lo; k <= hi; k++) {
        double re = 0.0, im = 0.0;
        int ph = 0;
        for (int n = 0; n < nfft; n++) {
            re += in[n] * co[ph]; im += in[n] * si[ph];
            ph += k; if (ph >= nfft) ph -= nfft;
        }
        out[2 * k] = (float) re; out[2 * k + 1] = (float) im;
    }
}
#endif
