// Developer tool (CPU machine only; tools/make_ref_fax_golden.py builds and runs it): the FAX extension's decoder as the reference
// runs it -- the class (extensions/FAX/FaxDecoder.h:33-138) and its methods (FaxDecoder.cpp:56-556) as the reference's own statements,
// cut at build time into a temporary directory.  Nothing of the reference's text enters the repository; only the data
// (tests/golden/fax_ref.npz) does.
//
// What this harness adds (none of the reference's headers is used):
//   * u1_t, s2_t, u4_t, TYPEREAL (float) with MSIN / MCOS / MSQRT, K_2PI, MIN, MAX_RX_CHANS as the pinned lines have them;
//   * `private` made public around the cut class, so that the state behind a line can be read;
//   * allocators that hand out ZEROS: operator new[] and kiwi_imalloc (csrc/kg_fax.h defines what the reference leaves to malloc as
//     zeros); kiwi_irealloc ends the run (every script stays under the first allocation of 256 lines);
//   * NextTaskFast(): "ProcessSamples 2" follows every DecodeFaxLine and closes the line's record; "FaxPhasingLinePosition" tells that
//     the position was asked for, and its place in phasingPos[];
//   * ext_send_msg() and ext_send_msg_data() recording the texts as flags and the row; rcprintf() taking the median triple of :239;
//   * median_i (support/misc.cpp:90-96) restated from the pinned lines (it also keeps phasingPos[0] of the line whose position the sort
//     is about to move);
//   * the commands of fax_msgs and fax_task (fax.cpp:85-88, :128-145, :160-162, :167-169) restated from the pinned lines.
//
//   fax_ref script.txt pool.bin out.bin
//       script lines:  C lpm imagewidth carrier deviation bandwidth headers phasing autostop debug nom srate    Configure with reset
//                      R srate     what ext_update_get_sample_rateHz answers from here on
//                      H shift     `SET fax_shift=`
//                      T           `SET fax_stop`
//                      B off       ProcessSamples(pool + off, 512, shift) (pool.bin: int16)
//       out.bin: per B int32 lines, per line 12 int32 (blk = 0, off, type, typecount, imageline, phasingLinesLeft, skip, phasing_pos,
//       flags, phasingSkipData, ten_pct, ninety_pct) and, under the row flag, 1 + imagewidth bytes.  Then the state (kg_fax_info of
//       include/kiwigpu.h) and m_samples[spl], m_demod_data[spl], the previous image line [imagewidth] (zeros while m_imageline is 0),
//       m_outImage[imagewidth].
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

typedef unsigned char u1_t;
typedef short s2_t;
typedef unsigned int u4_t;
#define TYPEREAL float
#define MSIN(x) sinf(x)
#define MCOS(x) cosf(x)
#define MSQRT(x) sqrtf(x)
#define K_2PI (2.0 * 3.14159265358979323846)
#define MIN(a, b) ((a) < (b) ? (a) : (b))
#define MAX_RX_CHANS 16
#define faxprintf(fmt, ...)
#define evLatency(...)
#define NextTaskFast(s) next_task(s)

void *operator new[](size_t n)
{
    void *p = calloc(n ? n : 1, 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void operator delete[](void *p) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

static int snd_rate;
static double cur_srate;
static int ev_dump;
static double ext_update_get_sample_rateHz(int) { return cur_srate; }
static void panic(const char *why) { fprintf(stderr, "panic: %s\n", why); exit(8); }
static void *kiwi_imalloc(const char *, size_t n) { return calloc(n ? n : 1, 1); }
static void *kiwi_irealloc(const char *, void *, size_t) { fprintf(stderr, "the script outgrew the first image allocation\n"); exit(9); return nullptr; }
static void kiwi_ifree(void *p, const char *) { free(p); }

enum { F_SPS_CHANGED = 1, F_AUTOSTOPPED_0 = 2, F_AUTOSTOPPED_1 = 4, F_PHASED = 8, F_ROW_SENT = 16, F_PHASING_REJECTED = 32, F_MEDIAN = 64 };
static int line_flags, line_pos_idx, line_pos0, line_med[3];
static std::vector<unsigned char> line_row;
static std::vector<unsigned char> sent;
static int nlines;
static void next_task(const char *s);

static int ext_send_msg(int, bool, const char *msg, ...)
{
    if (!strcmp(msg, "EXT fax_sps_changed")) line_flags |= F_SPS_CHANGED;
    else if (!strcmp(msg, "EXT fax_autostopped=0")) line_flags |= F_AUTOSTOPPED_0;
    else if (!strcmp(msg, "EXT fax_autostopped=1")) line_flags |= F_AUTOSTOPPED_1;
    else if (!strcmp(msg, "EXT fax_phased")) line_flags |= F_PHASED;
    else { fprintf(stderr, "unexpected ext_send_msg %s\n", msg); exit(7); }
    return 0;
}
static int ext_send_msg_data(int, bool, u1_t cmd, u1_t *bytes, int nbytes)
{
    if (line_flags & F_ROW_SENT) { fprintf(stderr, "two rows in a line\n"); exit(7); }
    line_flags |= F_ROW_SENT;
    line_row.assign(1, cmd);
    line_row.insert(line_row.end(), bytes, bytes + nbytes);
    return 0;
}
static void rcprintf(int, const char *fmt, ...)
{
    if (strncmp(fmt, "FAX L%d SET phasingSkipData", 27)) return;
    va_list ap;
    va_start(ap, fmt);
    (void) va_arg(ap, int);
    for (int k = 0; k < 3; k++) line_med[k] = va_arg(ap, int);
    va_end(ap);
    line_flags |= F_MEDIAN;
}
static int intcomp(const void *a, const void *b) { return *(const int *) a - *(const int *) b; }
static int median_i(int *i, int len, int *pct_1, int *pct_2)
{
    line_pos0 = i[0];
    qsort(i, len, sizeof *i, intcomp);
    if (pct_1) *pct_1 = i[(int) (len * ((float) *pct_1 / 100.0))];
    if (pct_2) *pct_2 = i[(int) (len * ((float) *pct_2 / 100.0))];
    return i[len / 2];
}

#define private public
#include "FAX_CUT_CLASS.inc"
#undef private

static FaxDecoder dec;                          // static: zeroed, as m_FaxDecoder[] is
void FaxDecoder::FileWrite(u1_t *, int) {}

#include "FAX_CUT_METHODS.inc"

static void next_task(const char *s)
{
    if (!strcmp(s, "FaxPhasingLinePosition")) line_pos_idx = dec.phasingLinesLeft - 1;
    if (strcmp(s, "ProcessSamples 2")) return;
    int pos = -1;
    if (line_pos_idx >= 0) pos = (line_flags & F_MEDIAN) ? line_pos0 : dec.phasingPos[line_pos_idx];
    if ((line_flags & F_MEDIAN) && (line_med[2] - line_med[1]) > dec.m_SamplesPerLine / 6) line_flags |= F_PHASING_REJECTED;
    const int med = line_flags & F_MEDIAN;
    const int32_t r[12] = {0, (int32_t) trunc(dec.m_fi), (int32_t) dec.lasttype, dec.typecount, dec.m_imageline, dec.phasingLinesLeft, dec.m_skip, pos, line_flags,
                           med ? line_med[0] : 0, med ? line_med[1] : 0, med ? line_med[2] : 0};
    sent.insert(sent.end(), (const unsigned char *) r, (const unsigned char *) r + sizeof r);
    if (line_flags & F_ROW_SENT) sent.insert(sent.end(), line_row.begin(), line_row.end());
    nlines++;
    line_flags = 0; line_pos_idx = -1;
}

static std::vector<unsigned char> slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<unsigned char> v;
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script.txt pool.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *of = fopen(argv[3], "wb");
    if (!sf || !of) return 2;
    std::vector<unsigned char> pool = slurp(argv[2]);
    const size_t npool = pool.size() / sizeof(s2_t);
    bool capture = false, configured = false;
    float shift = 0;
    line_pos_idx = -1;
    char line[256];
    while (fgets(line, sizeof line, sf)) {
        line[strcspn(line, "\n")] = 0;
        const char op = line[0];
        if (op == 'C') {
            int lpm, w, car, dev, bw, hdr, ph, as, dbg, nom;
            double sr;
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d %d %d %lf", &lpm, &w, &car, &dev, &bw, &hdr, &ph, &as, &dbg, &nom, &sr) != 11) return 3;
            snd_rate = nom;
            cur_srate = sr;
            dec.Configure(0, lpm, w, 8, car, dev, (FaxDecoder::firfilter::Bandwidth) bw, 15.0, hdr != 0, ph != 0, as != 0, dbg, true);
            capture = true; configured = true;
        } else if (op == 0 || op == '#') {
        } else if (op == 'R') {
            if (sscanf(line + 1, "%lf", &cur_srate) != 1) return 3;
        } else if (op == 'H') {
            if (sscanf(line + 1, "%f", &shift) != 1) return 3;
        } else if (op == 'T') {
            capture = false;                    // fax_close: the task is removed, fax_t is cleared
            shift = 0;
        } else if (op == 'B') {
            unsigned long off;
            if (sscanf(line + 1, "%lu", &off) != 1 || off + 512 > npool) return 3;
            sent.clear();
            nlines = 0;
            if (capture) {
                dec.ProcessSamples((s2_t *) pool.data() + off, 512, shift);
                shift = 0;
            }
            fwrite(&nlines, 4, 1, of);
            if (!sent.empty()) fwrite(sent.data(), 1, sent.size(), of);
        } else return 3;
    }
    if (!configured) return 5;
    // the state: kg_fax_info
    const double d[10] = {dec.m_SamplesPerSec_nom, dec.m_SamplesPerSec_frac, dec.m_SamplesPerSec_frac_prev, dec.m_SampleRateRatio, dec.m_fi,
                          dec.m_lineIncrFrac, dec.m_lineIncrAcc, dec.m_lineBlend, dec.m_carrier, dec.m_deviation};
    const int32_t n[20] = {dec.m_lpm, dec.m_imagewidth, (int32_t) dec.firfilters[0].bandwidth, dec.m_bIncludeHeadersInImages, dec.m_use_phasing, dec.m_autostop,
                           dec.m_autostopped, dec.m_debug, dec.m_bSkipHeaderDetection, dec.m_SamplesPerLine,
                           dec.m_skip, dec.m_samp_idx, (int32_t) dec.lasttype, dec.typecount, dec.m_imageline, dec.phasingLinesLeft, dec.phasingSkipData, dec.have_phasing,
                           dec.firfilters[0].current, capture ? 1 : 0};
    if (dec.firfilters[0].current != dec.firfilters[1].current || dec.firfilters[0].bandwidth != dec.firfilters[1].bandwidth) return 6;
    const float pq[2] = {dec.Iprev, dec.Qprev};
    fwrite(d, sizeof d, 1, of); fwrite(n, sizeof n, 1, of); fwrite(pq, sizeof pq, 1, of);
    fwrite(dec.firfilters[0].buffer, sizeof(float) * 17, 1, of); fwrite(dec.firfilters[1].buffer, sizeof(float) * 17, 1, of);
    fwrite(dec.phasingPos, sizeof(int) * 40, 1, of);
    const int32_t tail[2] = {0, 0};
    memcpy((void *) &tail[0], &shift, 4);
    fwrite(tail, sizeof tail, 1, of);
    const int spl = dec.m_SamplesPerLine, w = dec.m_imagewidth;
    fwrite(dec.m_samples, 2, spl, of);
    fwrite(dec.m_demod_data, 1, spl, of);
    std::vector<unsigned char> prev(w, 0);
    if (dec.m_imageline != 0 && dec.imgpos >= w) memcpy(prev.data(), dec.m_imgdata + dec.imgpos - w, w);
    fwrite(prev.data(), 1, w, of);
    fwrite(dec.m_outImage, 1, w, of);
    fclose(of);
    return 0;
}
