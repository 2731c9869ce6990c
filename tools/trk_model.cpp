// trk_model.cpp -- the LITERAL model the tracking channels (kg_trk) are held to: one call of edge() is one rising edge of `clk`,
// every register of verilog/gps/demod.v, cacode.v and of gps.v's pause counter is a variable of the same name, assigned from the
// values BEFORE the edge (non-blocking semantics: next-state copies, committed together), and the soft CPU's GPS_Method / CloseLoop /
// SetRate / set_gain / CmdSetSat / CmdSetPolarity (e_cpu/kiwi.gps.asm) run statement by statement on a little-endian byte memory
// laid out as STRUCT GPS_CHAN.  It shares no code with flydog_sdr_gps_amd/csrc/kg_trk.h (the closed form) and is slow on purpose.
//
// Fixed here because the reference leaves it open: registers without a reset value start at 0 and cg_en at 1; host
// commands fall between two edges; the E1B code memory delivers, at every full_chip, the chip at the NEW nchip; the firmware's words
// reach lo_rate / cg_rate at the edges ms0 + lo_delay / ms0 + cg_delay and it reads ser_iq as latched by that epoch's ms1; an ms0
// while a service is due replaces it; one record per completed service.
//
//   trk_model BITS CODES < script > text      (tests/trk_common.py writes the script and reads the text)
// BITS: the packed 1-bit stream, LSB first.  CODES: 4092-byte blocks of E1B chips.  Script lines:
//   N nchan lo_delay cg_delay | S ch word | C ch block | L ch rate | G ch rate | l ch ki kpmki | g ch ki kpmki | P ch pol | M mask
//   R | U ch count | O ch on | X nclocks | D | Q ch (CACODE's 1023 chips) | T freq err ki kpmki (CloseLoop alone)
// Output: per X, "E ch clock ip qp ie qe il ql lo_rate cg_rate flags" per record, channel by channel; per D, "C ch hex" per channel
// and "K clock replica...".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

enum { GPS_INTEG_BITS = 20, L1_CODELEN = 1023, E1B_CODELEN = 4092, MAX_NAV_BITS = 128, E1B_MODE = 0x800 };
static const uint32_t INTEG_MASK = (1u << GPS_INTEG_BITS) - 1;

// STRUCT GPS_CHAN: byte offsets
enum { ch_NAV_MS = 0, ch_NAV_BITS = 2, ch_NAV_GLITCH = 4, ch_NAV_PREV = 6, ch_NAV_BUF = 8, ch_CG_FREQ = 8 + 2 * (MAX_NAV_BITS / 16),
       ch_LO_FREQ = ch_CG_FREQ + 8, ch_IQ = ch_LO_FREQ + 8, ch_CG_GAIN = ch_IQ + 4 * 2 * 3, ch_LO_GAIN = ch_CG_GAIN + 4,
       ch_unlocked = ch_LO_GAIN + 4, ch_E1B_mode = ch_unlocked + 2, ch_LO_polarity = ch_E1B_mode + 2, sizeof_GPS_CHAN = ch_LO_polarity + 2 };

struct Record { uint64_t clock; int32_t v[6]; uint32_t lo, cg, flags; };

struct Demod {
    // demod.v
    int e1b_mode = 0, g2_init = 0, init = 0;
    int cg_en = 1;
    uint32_t lo_rate = 0, lo_phase = 0, cg_rate = 0, cg_phase = 0;
    int chips = 0, cg_p = 0, ms0 = 0, ms1 = 0, cg_l = 0, e1b_latched_code = 0, nchip = 0;
    int lsb = 0, die = 0, dqe = 0, dip = 0, dqp = 0, dil = 0, dql = 0;
    uint32_t ie = 0, qe = 0, ip = 0, qp = 0, il = 0, ql = 0;
    uint32_t ser_iq[6] = {0, 0, 0, 0, 0, 0};      // {ip, qp, ie, qe, il, ql}
    // cacode.v: g[i], i = 1..10
    int g1[11] = {0}, g2[11] = {0};               // index 0 unused
    // the soft CPU
    uint8_t mem[sizeof_GPS_CHAN] = {0};
    int loop_on = 1, lo_due = 0, cg_due = 0;      // 0: none
    uint64_t ms1_clock = 0;
};

static int nchan, lo_delay, cg_delay;
static std::vector<Demod> D;
static std::vector<std::vector<uint8_t>> e1b_mem;     // the E1B code memory's column of each channel
static std::vector<std::vector<Record>> recs;
static uint32_t cg_cnt = 0, chan_mask = 0;        // gps.v
static uint64_t clk_count = 0;

// ---- the soft CPU's memory and ALU
static uint32_t fetch16(Demod &d, int a) { return d.mem[a] | (d.mem[a + 1] << 8); }
static void store16(Demod &d, int a, uint32_t v) { d.mem[a] = v & 0xFF; d.mem[a + 1] = (v >> 8) & 0xFF; }
static void store32(Demod &d, int a, uint32_t v) { store16(d, a, v & 0xFFFF); store16(d, a + 2, v >> 16); }
static uint64_t fetch64(Demod &d, int a)
{
    uint64_t v = 0;
    for (int i = 3; i >= 0; i--) v = (v << 16) | fetch16(d, a + 2 * i);
    return v;
}
static void store64(Demod &d, int a, uint64_t v) { for (int i = 0; i < 4; i++) store16(d, a + 2 * i, (uint32_t) ((v >> (16 * i)) & 0xFFFF)); }
static int32_t sext20_32(uint32_t v) { return (v & 0x80000) ? (int32_t) (v | 0xFFF00000u) : (int32_t) (v & 0xFFFFF); }
// cpu.v: xa20 = nos[19:0], xb20 = tos[19:0], signed 20 x 20 -> prod40, sign-extended to 64 bits
static uint64_t mult20(uint32_t nos, uint32_t tos)
{
    const int64_t prod40 = (int64_t) sext20_32(nos & 0xFFFFF) * (int64_t) sext20_32(tos & 0xFFFFF);
    return (uint64_t) prod40;
}
static uint64_t shl64_n(uint64_t v, uint32_t n) { while (n--) v <<= 1; return v; }

static uint32_t CloseLoop(Demod &d, uint64_t err, int freq, int gain)
{
    const uint32_t ki = fetch16(d, gain);
    const uint64_t eki = shl64_n(err, ki);
    const uint64_t cur = fetch64(d, freq);
    const uint64_t newF = cur + eki;
    store64(d, freq, newF);
    const uint32_t kp_m_ki = fetch16(d, gain + 2);
    const uint64_t ekp = shl64_n(eki, kp_m_ki);
    const uint64_t nco64 = newF + ekp;
    return (uint32_t) (nco64 >> 32);
}

static void GPS_Method_lo(Demod &d)
{
    const uint32_t ip = d.ser_iq[0], qp = d.ser_iq[1];
    store32(d, ch_IQ, (uint32_t) sext20_32(ip));
    store32(d, ch_IQ + 4, (uint32_t) sext20_32(qp));
    if (!d.loop_on) return;
    d.lo_rate = CloseLoop(d, mult20(ip, qp), ch_LO_FREQ, ch_LO_GAIN);           // wrReg SET_LO_NCO
}

static uint64_t GetPower(uint32_t i, uint32_t q) { return mult20(i, i) + mult20(q, q); }

static void GPS_Method_cg(Demod &d, std::vector<Record> &out)
{
    const uint32_t Inav = (d.ser_iq[0] >> 19) & 1;
    const uint64_t pp = mult20(d.ser_iq[1], d.ser_iq[1]) + mult20(d.ser_iq[0], d.ser_iq[0]);
    const uint64_t pe = GetPower(d.ser_iq[2], d.ser_iq[3]);
    store64(d, ch_IQ + 8, pe);
    const uint32_t s_pe = ((int64_t) (pp - pe) < 0) ? 0x8000 : 0;               // sgn64_16
    const uint64_t pl = GetPower(d.ser_iq[4], d.ser_iq[5]);
    store64(d, ch_IQ + 16, pl);
    const uint32_t s_pl = ((int64_t) (pp - pl) < 0) ? 0x8000 : 0;
    store16(d, ch_unlocked, s_pl | s_pe);
    uint64_t err = pe - pl;
    if (fetch16(d, ch_E1B_mode) != 0) {                                         // E1B_CG_loop
        const uint32_t pol = fetch16(d, ch_LO_polarity);
        if (pol != 0) {
            const uint64_t ACF = err;
            const uint64_t AACF = ((int64_t) ACF < 0) ? (uint64_t) (-(int64_t) ACF) : ACF;
            if (pol - 1 == 0) err = ACF + AACF; else err = ACF - AACF;
        }
    }
    if (d.loop_on) d.cg_rate = CloseLoop(d, err, ch_CG_FREQ, ch_CG_GAIN);       // wrReg SET_CG_NCO
    bool NavSave = fetch16(d, ch_E1B_mode) != 0;
    if (!NavSave) {
        const uint32_t prev = fetch16(d, ch_NAV_PREV);
        if (prev - Inav != 0) {                                                 // NavNotSame
            store16(d, ch_NAV_PREV, Inav);
            if (fetch16(d, ch_NAV_MS) != 0) store16(d, ch_NAV_GLITCH, fetch16(d, ch_NAV_GLITCH) + 1);
            store16(d, ch_NAV_MS, 1);                                           // NavEdge
        } else {                                                                // NavSame
            const uint32_t ms = fetch16(d, ch_NAV_MS);
            if (ms - 19 == 0) NavSave = true;
            else store16(d, ch_NAV_MS, ms + 1);
        }
    }
    if (NavSave) {
        store16(d, ch_NAV_MS, 0);
        const uint32_t cnt = fetch16(d, ch_NAV_BITS);
        store16(d, ch_NAV_BITS, (cnt + 1) & (MAX_NAV_BITS - 1));
        const int ptr = ch_NAV_BUF + ((cnt >> 4) << 1);
        store16(d, ptr, (fetch16(d, ptr) << 1) + Inav);
    }
    Record r;
    r.clock = d.ms1_clock;
    for (int i = 0; i < 6; i++) r.v[i] = sext20_32(d.ser_iq[i]);
    r.lo = d.lo_rate; r.cg = d.cg_rate;
    r.flags = (fetch16(d, ch_unlocked) ? 1 : 0) | (Inav << 1);
    out.push_back(r);
}

// ---- one rising edge of clk for the whole bank
static void edge(int sample)
{
    // gps.v:190-200
    const uint32_t dec = (cg_cnt - 1) & 0x1FFFF;
    const int cg_resume = (dec >> 16) & 1;
    const uint32_t cg_nxt = dec & 0xFFFF;
    for (int ch = 0; ch < nchan; ch++) {
        Demod &d = D[ch];
        Demod n = d;                                    // next state: every right-hand side below reads d
        // pause
        if (!d.cg_en) n.cg_en = cg_resume;
        // NCOs: the 30-bit adder and the two carry-chain cells
        const uint32_t s30 = (d.cg_phase & 0x3FFFFFFF) + (d.cg_rate & 0x3FFFFFFF);
        const int quarter_chip = (s30 >> 30) & 1;
        const int a30 = (d.cg_phase >> 30) & 1, b30 = (d.cg_rate >> 30) & 1, ci30 = quarter_chip;
        const int d30 = a30 ^ b30;
        const int sum30 = d30 ^ ci30, half_chip = d30 ? ci30 : a30;
        const int a31 = (d.cg_phase >> 31) & 1, b31 = (d.cg_rate >> 31) & 1, ci31 = half_chip;
        const int d31 = a31 ^ b31;
        const int sum31 = d31 ^ ci31, full_chip = d31 ? ci31 : a31;
        const uint32_t cg_sum = (s30 & 0x3FFFFFFF) | ((uint32_t) sum30 << 30) | ((uint32_t) sum31 << 31);
        const int full_chip_en = full_chip & d.cg_en;
        n.lo_phase = d.lo_phase + d.lo_rate;
        if (d.cg_en) n.cg_phase = cg_sum;
        n.ms1 = d.ms0;
        // cacode.v
        const int T0 = (d.init >> 4) & 15, T1 = d.init & 15;
        const int ca_chip = d.g2_init ? (d.g1[10] ^ d.g2[10]) : (d.g1[10] ^ d.g2[T0 <= 10 ? T0 : 0] ^ d.g2[T1 <= 10 ? T1 : 0]);
        if (full_chip_en) {
            for (int i = 10; i >= 2; i--) { n.g1[i] = d.g1[i - 1]; n.g2[i] = d.g2[i - 1]; }
            n.g1[1] = d.g1[3] ^ d.g1[10];
            n.g2[1] = d.g2[2] ^ d.g2[3] ^ d.g2[6] ^ d.g2[8] ^ d.g2[9] ^ d.g2[10];
        }
        // code and epoch
        const int boc11 = (d.cg_phase >> 31) & 1;
        const int e1b_chip = d.e1b_latched_code ^ boc11;
        const int cg_e = d.e1b_mode ? e1b_chip : ca_chip;
        if (d.e1b_mode) {
            int nchip_nxt = d.nchip;
            if (full_chip_en) nchip_nxt = (d.nchip == E1B_CODELEN - 1) ? 0 : ((d.nchip + 1) & 0xFFF);
            n.nchip = nchip_nxt;
            if (full_chip) {
                n.e1b_latched_code = e1b_mem[ch][nchip_nxt % E1B_CODELEN];         // what the code memory is built to deliver
                n.cg_l = d.cg_p;
            }
            if (quarter_chip && !full_chip) {
                if (half_chip) {
                    n.cg_l = d.cg_p;
                    n.chips = d.nchip;
                    n.ms0 = (d.nchip == 0);
                } else {
                    n.cg_p = cg_e;
                }
            } else {
                n.ms0 = 0;
            }
        } else {
            if (full_chip_en) n.nchip = (d.nchip == L1_CODELEN - 1) ? 0 : ((d.nchip + 1) & 0xFFF);
            if (half_chip) {
                if (full_chip) {
                    n.cg_l = d.cg_p;
                } else {
                    n.cg_p = cg_e;
                    n.chips = d.nchip;
                    n.ms0 = (d.nchip == 0);
                }
            } else {
                n.ms0 = 0;
            }
        }
        // final LO
        const int lo_sin = 0xC, lo_cos = 0x6;
        const int LO_I = (lo_sin >> (d.lo_phase >> 30)) & 1, LO_Q = (lo_cos >> (d.lo_phase >> 30)) & 1;
        // mixers
        n.die = sample ^ cg_e ^ LO_I;    n.dqe = sample ^ cg_e ^ LO_Q;
        n.dip = sample ^ d.cg_p ^ LO_I;  n.dqp = sample ^ d.cg_p ^ LO_Q;
        n.dil = sample ^ d.cg_l ^ LO_I;  n.dql = sample ^ d.cg_l ^ LO_Q;
        // filters: {20{d}} + lsb
#define FILT(acc_, bit_) n.acc_ = ((d.ms1 ? 0 : d.acc_) + (d.bit_ ? INTEG_MASK : 0) + d.lsb) & INTEG_MASK
        FILT(ie, die); FILT(qe, dqe); FILT(ip, dip); FILT(qp, dqp); FILT(il, dil); FILT(ql, dql);
#undef FILT
        n.lsb = d.ms1 ? 0 : !d.lsb;
        if (d.ms1) {
            n.ser_iq[0] = d.ip; n.ser_iq[1] = d.qp; n.ser_iq[2] = d.ie; n.ser_iq[3] = d.qe; n.ser_iq[4] = d.il; n.ser_iq[5] = d.ql;
            n.ms1_clock = clk_count;
        }
        const bool srq = n.ms0 != 0;
        d = n;
        // the soft CPU, after the edge: its register writes act from the next edge on
        if (d.lo_due > 0 && --d.lo_due == 0) GPS_Method_lo(d);
        if (d.cg_due > 0 && --d.cg_due == 0) GPS_Method_cg(d, recs[ch]);
        if (srq) { d.lo_due = lo_delay; d.cg_due = cg_delay; }
    }
    cg_cnt = cg_nxt;
    clk_count++;
}

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: trk_model BITS CODES < script\n"); return 2; }
    const std::vector<uint8_t> bits = slurp(argv[1]), codes = slurp(argv[2]);
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char op = 0;
        long long a = 0, b = 0, c = 0;
        if (sscanf(line, " %c %lld %lld %lld", &op, &a, &b, &c) < 1) continue;
        if (op == 'T') {                                                  // CloseLoop alone: T freq err ki kp-ki -> "T newfreq nco"
            unsigned long long f = 0; long long e = 0; int ki = 0, kpm = 0;
            sscanf(line, " %c %llu %lld %d %d", &op, &f, &e, &ki, &kpm);
            Demod t;
            store64(t, ch_CG_FREQ, f); store16(t, ch_CG_GAIN, (uint32_t) ki); store16(t, ch_CG_GAIN + 2, (uint32_t) kpm);
            const uint32_t nco = CloseLoop(t, (uint64_t) e, ch_CG_FREQ, ch_CG_GAIN);
            printf("T %llu %u\n", (unsigned long long) fetch64(t, ch_CG_FREQ), nco);
            continue;
        }
        if (op == 'N') { nchan = (int) a; lo_delay = (int) b; cg_delay = (int) c; D.assign(nchan, Demod());
                        e1b_mem.assign(nchan, std::vector<uint8_t>(E1B_CODELEN, 0)); recs.assign(nchan, std::vector<Record>()); continue; }
        if (op != 'M' && op != 'R' && op != 'X' && op != 'D' && (a < 0 || a >= nchan)) { fprintf(stderr, "bad channel: %s", line); return 2; }
        Demod *d = (op != 'M' && op != 'R' && op != 'X' && op != 'D') ? &D[a] : nullptr;
        switch (op) {
        case 'S':                                                       // CmdSetSat
            d->e1b_mode = (b >> 11) & 1; d->g2_init = (b >> 10) & 1; d->init = (int) (b & 0x3FF);
            store16(*d, ch_E1B_mode, (uint32_t) b & E1B_MODE);
            break;
        case 'C':
            if ((size_t) (b + 1) * E1B_CODELEN > codes.size()) { fprintf(stderr, "no code block %lld\n", b); return 2; }
            e1b_mem[a].assign(codes.begin() + b * E1B_CODELEN, codes.begin() + (b + 1) * E1B_CODELEN);
            break;
        case 'L': store64(*d, ch_LO_FREQ, (uint64_t) (uint32_t) b << 32); d->lo_rate = (uint32_t) b; break;     // SetRate
        case 'G': store64(*d, ch_CG_FREQ, (uint64_t) (uint32_t) b << 32); d->cg_rate = (uint32_t) b; break;
        case 'l': store32(*d, ch_LO_GAIN, (uint32_t) (b + (c << 16))); break;                                   // set_gain: ki + ((kp-ki)<<16)
        case 'g': store32(*d, ch_CG_GAIN, (uint32_t) (b + (c << 16))); break;
        case 'P': store16(*d, ch_LO_polarity, (uint32_t) b); break;
        case 'M': chan_mask = (uint32_t) a; break;
        case 'R':                                                       // CmdSample: chan_rst = sampler_rst & ~chan_mask
            for (int ch = 0; ch < nchan; ch++) {
                if ((chan_mask >> ch) & 1) continue;
                Demod &r = D[ch];
                r.cg_phase = 0; r.nchip = 0;
                for (int i = 1; i <= 10; i++) { r.g1[i] = 1; r.g2[i] = r.g2_init ? (r.init >> (i - 1)) & 1 : 1; }
            }
            break;
        case 'Q': {                                                     // the 1023 chips CACODE gives after rst, rd once per chip
            int g1[11], g2[11];
            for (int i = 1; i <= 10; i++) { g1[i] = 1; g2[i] = d->g2_init ? (d->init >> (i - 1)) & 1 : 1; }
            const int T0 = (d->init >> 4) & 15, T1 = d->init & 15;
            printf("Q %lld ", a);
            for (int k = 0; k < L1_CODELEN; k++) {
                printf("%d", d->g2_init ? (g1[10] ^ g2[10]) : (g1[10] ^ g2[T0 <= 10 ? T0 : 0] ^ g2[T1 <= 10 ? T1 : 0]));
                const int n1 = g1[3] ^ g1[10], n2 = g2[2] ^ g2[3] ^ g2[6] ^ g2[8] ^ g2[9] ^ g2[10];
                for (int i = 10; i >= 2; i--) { g1[i] = g1[i - 1]; g2[i] = g2[i - 1]; }
                g1[1] = n1; g2[1] = n2;
            }
            printf("\n");
            break;
        }
        case 'U': d->cg_en = 0; cg_cnt = (uint32_t) b & 0xFFFF; break;   // SET_PAUSE
        case 'O': d->loop_on = b != 0; break;
        case 'X':
            for (long long k = 0; k < a; k++) {
                const uint64_t bit = clk_count;
                if ((bit >> 3) >= bits.size()) { fprintf(stderr, "stream too short\n"); return 2; }
                edge((bits[bit >> 3] >> (bit & 7)) & 1);
            }
            for (int ch = 0; ch < nchan; ch++) {
                for (const Record &r : recs[ch])
                    printf("E %d %llu %d %d %d %d %d %d %u %u %u\n", ch, (unsigned long long) r.clock, r.v[0], r.v[1], r.v[2], r.v[3], r.v[4], r.v[5],
                           r.lo, r.cg, r.flags);
                recs[ch].clear();
            }
            break;
        case 'D':
            for (int ch = 0; ch < nchan; ch++) {
                printf("C %d ", ch);
                for (int i = 0; i < sizeof_GPS_CHAN; i++) printf("%02x", D[ch].mem[i]);
                printf("\n");
            }
            printf("K %llu", (unsigned long long) clk_count);
            for (int ch = 0; ch < nchan; ch++) {
                const Demod &r = D[ch];                                 // demod.v:290-292
                const uint32_t replica = ((((r.cg_phase >> 31) & 1) ^ 1) << 17) | (((r.cg_phase >> 26) & 0x1F) << 12) | ((r.chips & 0x3FF) << 2) |
                                         ((r.chips >> 10) & 3);
                printf(" %u", replica);
            }
            printf("\n");
            break;
        default: fprintf(stderr, "bad line: %s", line); return 2;
        }
    }
    return 0;
}
