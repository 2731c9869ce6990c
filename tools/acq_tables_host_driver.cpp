// Host driver for tests/test_acq_horner_cpu.py: writes the row-constant table of the C/A correlator's last pass
// (kg_acq_row_consts, csrc/kg_acq_tables.h -- the builder acq_init() calls) as raw fp32 (re, im) pairs.
// usage: acq_tables_host_driver P out.bin
//        acq_tables_host_driver mid out.bin     the restart factors of the P = 16 Horner chain (kg_acq_mid_factors), [4][256]
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../flydog_sdr_gps_amd/csrc/kg_acq_tables.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s P out.bin\n", argv[0]); return 2; }
    if (argv[1][0] == 'm') {
        std::vector<float> mid(4 * 256 * 2);
        kg_acq_mid_factors(65536, mid.data());
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(mid.data(), sizeof(float), mid.size(), f) != mid.size() || fclose(f) != 0) { perror(argv[2]); return 1; }
        return 0;
    }
    const int P = atoi(argv[1]);
    if (P != 4 && P != 16) { fprintf(stderr, "P = 4 or 16\n"); return 2; }
    std::vector<float> tab((size_t) P * KG_ACQ_ROWK * 2);
    kg_acq_row_consts(P, tab.data());
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(tab.data(), sizeof(float), tab.size(), f) != tab.size() || fclose(f) != 0) { perror(argv[2]); return 1; }
    return 0;
}
