// Host driver of csrc/kg_spec.h (tests/spec_common.py compiles it with g++ -O2 -ffp-contract=off, the reference's flags): the audio
// spectrum row, the 125 ms limiter and the emission rule, with the modes, the script language and the output layouts of
// tools/ref/ref_spec_main.cpp.
//   spec_host_driver rows    in.bin out.bin           every spectrum with the passband scale, then the channel-null one
//   spec_host_driver limiter clocks.bin out.bin       one connection, one call per u32 clock: int32 fired, u32 last_ms
//   spec_host_driver emit    script.txt blocks.bin out.bin
//       the command semantics of kg_rxbank_set_spec and of a host that sends kg_post_set_sam_mparam (n == 5, SAM family) and
//       kg_post_set_mode for a mode command that changes the mode or has n == 5 -- each of which clears the bank's mirror -- and
//       the bank's walk over one receiver's sound blocks
#include "../flydog_sdr_gps_amd/csrc/kg_spec.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace kg_spec;

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
    if (argc < 4) { fprintf(stderr, "usage: %s rows|limiter|emit ...\n", argv[0]); return 2; }
    const size_t SPEC = WIDTH * 2 * sizeof(float);
    if (!strcmp(argv[1], "rows")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % SPEC) return 2;
        unsigned char fft[WIDTH];
        for (size_t r = 0; r < in.size() / SPEC; r++)
            for (int inst = PASSBAND; inst <= CHAN_NULL; inst++) {
                row((const float *) (in.data() + r * SPEC), inst, fft);
                fwrite(fft, 1, WIDTH, of);
            }
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "limiter")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        FILE *of = fopen(argv[3], "wb");
        if (!of || in.size() % 4) return 2;
        uint32_t last = 0;
        for (size_t k = 0; k < in.size() / 4; k++) {
            uint32_t now;
            memcpy(&now, in.data() + 4 * k, 4);
            const int fired = due(&last, now);
            fwrite(&fired, 4, 1, of);
            fwrite(&last, 4, 1, of);
        }
        fclose(of);
        return 0;
    }
    if (!strcmp(argv[1], "emit") && argc == 5) {
        FILE *sf = fopen(argv[2], "r"), *of = fopen(argv[4], "wb");
        if (!sf || !of) return 2;
        const std::vector<unsigned char> blocks = slurp(argv[3]);
        size_t next = 0;
        enum { MODE_SAM = 11, MODE_QAM = 15 };                         // rx/mode.h:69-70: SAM, SAU, SAL, SAS, QAM
        int spec_on = 0, mode = -1, sam_mparam = 0;
        emit_t mirror;
        emit_clear(mirror);
        char line[256];
        unsigned char fft[WIDTH];
        while (fgets(line, sizeof line, sf)) {
            const char op = line[0];
            if (op == 'P') {
                int n;
                if (sscanf(line + 1, "%d", &n) != 1) return 3;
                spec_on = cmd_on(n);
            } else if (op == 'M') {
                int m, mp, n5;
                if (sscanf(line + 1, "%d %d %d", &m, &mp, &n5) != 3) return 3;
                if (mode != m || n5) {
                    if (m >= MODE_SAM && m <= MODE_QAM && n5) { sam_mparam = mp & 0xf; emit_clear(mirror); }     // kg_post_set_sam_mparam
                    mode = m;
                    emit_clear(mirror);                                                                      // kg_post_set_mode
                }
            } else if (op == 'B') {
                const bool sam_family = mode >= MODE_SAM && mode <= MODE_QAM, sam_null = mode == MODE_SAM && (sam_mparam & 3);
                const rows_t r = emit_block(mirror, spec_on != 0, sam_family, sam_null);
                const int nr = r.passband + r.chan_null;
                fwrite(&nr, 4, 1, of);
                for (int inst = PASSBAND; inst <= CHAN_NULL; inst++) {
                    if (inst == CHAN_NULL && !sam_null) continue;       // the second filter is fed in channel-null SAM only
                    if ((next + 1) * SPEC > blocks.size()) return 4;
                    const int blk = (int) next++;                       // every fill is handed a block, sent or not
                    if (!(inst == PASSBAND ? r.passband : r.chan_null)) continue;
                    const int iv[3] = {inst, inst, blk};                // the scale is the instance's
                    row((const float *) (blocks.data() + (size_t) blk * SPEC), inst, fft);
                    fwrite(iv, sizeof iv, 1, of);
                    fwrite(fft, 1, WIDTH, of);
                }
            } else if (op != '\n' && op != '#') return 3;
        }
        fclose(of);
        return 0;
    }
    return 2;
}
