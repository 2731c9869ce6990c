// Developer tool (CPU machine only; tools/make_ref_nb_golden.py builds and runs it): CuteSDR's CNoiseProc (rx/CuteSDR/noiseproc.cpp,
// linked where it lies) driven as its two call sites drive it: the audio blanker as rx/rx_sound.cpp:597 calls it (ProcessBlanker, in
// place on the unpacked block) and the waterfall blanker as rx/rx_waterfall.cpp:1092 / :1098 do (SetupBlanker("WF", WF_C_NSAMPS,
// ...), ProcessBlankerOneShot(WF_C_NSAMPS, ...) in place on the windowed frame).  Those statements are cut from
// the reference at build time (NB_CUT_SND, NB_CUT_WF_SETUP, NB_CUT_WF_ONESHOT) and checked against their text by the generator.
// Nothing of the reference's text enters the repository; only the data (tests/golden/nb_ref.npz) does.
//
//   nb_ref script.txt in.bin out.bin
// script lines:
//   U rate gate th   -> m_NoiseProc_snd[0].SetupBlanker("SND", rate, {gate, th, 0...}) (values as text: strtof)
//   B n              -> the audio call site on the next n complex floats of in.bin; out: the n complex floats after it
//   W gate th        -> the waterfall's SetupBlanker (rx_waterfall.cpp:1092)
//   F                -> the waterfall's ProcessBlankerOneShot on the next 8192 complex floats of in.bin; out: the frame after it
//   S / T            -> the audio / waterfall blanker's state: int32 m_Mptr, m_Dptr, m_BlankCounter, m_MagSamples, m_DelaySamples,
//                       m_GateSamples; float m_Ratio, m_MagAveSum
#define private public           // CNoiseProc's members, for the end states only
#include "datatypes.h"
#include "rx_noise.h"
#include "noiseproc.h"
#undef private
#undef printf
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WF_C_NSAMPS 8192
static CNoiseProc m_NoiseProc_snd[1], m_NoiseProc_wf[1];

static void dump(FILE *f, const CNoiseProc &p)
{
    const int iv[6] = {p.m_Mptr, p.m_Dptr, p.m_BlankCounter, p.m_MagSamples, p.m_DelaySamples, p.m_GateSamples};
    const float fv[2] = {p.m_Ratio, p.m_MagAveSum};
    fwrite(iv, sizeof iv, 1, f);
    fwrite(fv, sizeof fv, 1, f);
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s script in.bin out.bin\n", argv[0]); return 2; }
    FILE *sf = fopen(argv[1], "r"), *inf = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!sf || !inf || !outf) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int rx_chan = 0;
    static TYPECPX in_samps_c[1 << 16];
    static struct { TYPEREAL hw_c_samps[WF_C_NSAMPS][2]; } fft_s;
    auto *fft = &fft_s;                                                                      // rx_waterfall.cpp's fft->hw_c_samps
    TYPEREAL snd_param[NOISE_PARAMS];
    struct { TYPEREAL nb_param[NOISE_TYPES][NOISE_PARAMS]; } wf_inst, *wf = &wf_inst;      // wf_inst_t's nb_param only
    char line[1024], a[64], b[64], c[64];
    while (fgets(line, sizeof line, sf)) {
        const char op = line[0];
        if (op == 'U') {
            if (sscanf(line + 1, "%63s %63s %63s", a, b, c) != 3) return 3;
            memset(snd_param, 0, sizeof snd_param);
            const float frate = strtof(a, nullptr);
            snd_param[NB_GATE] = strtof(b, nullptr); snd_param[NB_THRESHOLD] = strtof(c, nullptr);
            m_NoiseProc_snd[rx_chan].SetupBlanker("SND", frate, snd_param);
        } else if (op == 'B') {
            int ns_in;
            if (sscanf(line + 1, "%d", &ns_in) != 1 || ns_in < 0 || ns_in > (1 << 16)) return 3;
            if (fread(in_samps_c, sizeof(TYPECPX), ns_in, inf) != (size_t) ns_in) return 4;
#include "NB_CUT_SND.inc"
            fwrite(in_samps_c, sizeof(TYPECPX), ns_in, outf);
        } else if (op == 'W') {
            if (sscanf(line + 1, "%63s %63s", b, c) != 2) return 3;
            memset(wf, 0, sizeof *wf);
            wf->nb_param[NB_BLANKER][NB_GATE] = strtof(b, nullptr); wf->nb_param[NB_BLANKER][NB_THRESHOLD] = strtof(c, nullptr);
            u4_t srate = WF_C_NSAMPS;
#include "NB_CUT_WF_SETUP.inc"
        } else if (op == 'F') {
            if (fread(fft->hw_c_samps, sizeof(TYPECPX), WF_C_NSAMPS, inf) != WF_C_NSAMPS) return 4;
#include "NB_CUT_WF_ONESHOT.inc"
            fwrite(fft->hw_c_samps, sizeof(TYPECPX), WF_C_NSAMPS, outf);
        } else if (op == 'S') {
            dump(outf, m_NoiseProc_snd[rx_chan]);
        } else if (op == 'T') {
            dump(outf, m_NoiseProc_wf[rx_chan]);
        } else if (op != '\n' && op != '#') return 3;
    }
    fclose(outf);
    return 0;
}
