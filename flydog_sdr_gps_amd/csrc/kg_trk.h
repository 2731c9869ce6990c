// kg_trk.h -- the arithmetic of one GPS tracking channel (verilog/gps/demod.v, cacode.v, e1bcode.v as its round-robin memory is
// built to deliver, gps.v:190-200; e_cpu/kiwi.gps.asm GPS_Method and CloseLoop) in CLOSED FORM, for the device (kg_trk.hip) and,
// compiled by a host compiler, for tools/trk_host_driver.cpp -- as kg_nbw.h is.  The literal clock-by-clock model it is held to
// (tools/trk_model.cpp) shares nothing with this file.
//
// Clocks.  "Edge k" is the k-th rising clock edge the bank consumes; sample bit k is what `sample` holds before it.  With a constant
// cg_rate r and cg_phase p0 before edge 0 of a segment, A(k) = p0 + k r (not reduced) gives everything before edge k:
//   carries out of bit 31 (full_chip) at the edges 0..k-1      A(k) >> 32
//   carries into bit 31 (half_chip)                            (A(k) >> 31) - (p0 >> 31)
//   carries into bit 30 (quarter_chip)                         (A(k) >> 30) - (p0 >> 30)
// because an edge j carries into bit b exactly when a multiple of 2^b lies in (A(j), A(j+1)].  r < 2^29 makes the three classes
// nested (full => half => quarter) and at least two edges apart, so ms0 stands for one edge; r >= 2^27 bounds a chip to 32 edges and
// an epoch to 32736 (kg_trk_set_rate_cg refuses anything else, and run() stops a channel whose own loop writes such a word).  P and L are E delayed to the last qualifying crossing:
//   C/A  P <- E at the odd multiples of 2^31 (chips, ms0 there); L <- P at the multiples of 2^32
//   E1B  P <- E at the odd multiples of 2^30; L <- P at the even ones; chips, ms0 at 2 mod 4; the latched code <- memory[nchip'] at 0 mod 4
// While the generator is paused the phase stands still and the three carries, being combinational, hold: their latchings then repeat
// every edge and are idempotent from the second edge on (the frozen branch of run()).  A held ms0 is the one thing that is not (it would
// restart the integrators every clock); the host side refuses the pause that would cause it (kg_trk.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KG_TRK_FN __host__ __device__ static inline
#else
#define KG_TRK_FN static inline
#endif

namespace kg_trk_cf {

enum { L1_CODELEN = 1023, E1B_CODELEN = 4092, INTEG_BITS = 20, REPL_BITS = 18, MAX_NAV_BITS = 128, E1B_MODE = 0x800, G2_INIT = 0x400,
       CHAN_BYTES = 78, TABLE_WORDS = 128 };

// struct GPS_CHAN, kiwi.gps.asm:31-45: the soft CPU's memory is little endian, so the first CHAN_BYTES bytes of this are the record
struct gps_chan {
    uint16_t nav_ms, nav_bits, nav_glitch, nav_prev, nav_buf[MAX_NAV_BITS / 16];
    uint64_t cg_freq, lo_freq;
    uint32_t iq[6];                       // ip, qp (sign-extended), pe (64 bits), pl (64 bits)
    uint16_t cg_gain[2], lo_gain[2], unlocked, e1b_mode, lo_polarity;
    uint16_t pad_;
};

struct chan {
    gps_chan fw;
    uint32_t lo_rate, lo_phase, cg_rate, cg_phase;
    uint32_t nchip, chips;
    uint32_t integ[6], ser[6];            // order ip qp ie qe il ql, INTEG_BITS wide
    uint32_t sat;                         // the 12-bit word of op_set_sat
    uint32_t d;                           // the six mixer registers, bit i of the order above
    uint32_t cg_en, cg_p, cg_l, lat, lsb;
    int32_t ms1_due, lo_due, cg_due;      // edges left before the edge that sees ms1 / through the edge that writes the NCO; -1: none
    uint32_t loop_on, have_sat, seeded, have_code;
    uint32_t fault;                       // the code loop wrote a word outside [2^27, 2^29): the channel stands from there on
    uint32_t lo_delay, cg_delay;          // edges from the one that sets ms0 to the ones that write the NCO words
    uint64_t ms1_clock;
};

struct chan_tab { uint32_t w[TABLE_WORDS]; };   // chip n of the epoch at bit n: C/A from the generator's seed, E1B the memory code

struct epoch {                            // == kg_trk_epoch (include/kiwigpu.h)
    uint64_t clock;
    int32_t ip, qp, ie, qe, il, ql;
    uint32_t lo_rate, cg_rate, flags, pad_;
};

KG_TRK_FN int32_t sext20(uint32_t v) { return (int32_t) (v << 12) >> 12; }
KG_TRK_FN int64_t mult20(uint32_t a, uint32_t b) { return (int64_t) sext20(a) * (int64_t) sext20(b); }   // cpu.v:179,224,234-236
KG_TRK_FN uint64_t shl64_n(uint64_t v, unsigned n) { return n >= 64 ? 0 : v << n; }

// CloseLoop, kiwi.gps.asm:73-97
KG_TRK_FN uint32_t close_loop(uint64_t *freq, const uint16_t *gain, uint64_t err)
{
    const uint64_t eki = shl64_n(err, gain[0]);
    const uint64_t nf = *freq + eki;
    *freq = nf;
    return (uint32_t) ((nf + shl64_n(eki, gain[1])) >> 32);
}

// GPS_Method up to the LO loop (:192-220); writes SET_LO_NCO
KG_TRK_FN void service_lo(chan &c)
{
    const uint32_t ip = c.ser[0], qp = c.ser[1];
    c.fw.iq[0] = (uint32_t) sext20(ip);
    c.fw.iq[1] = (uint32_t) sext20(qp);
    if (c.loop_on) c.lo_rate = close_loop(&c.fw.lo_freq, c.fw.lo_gain, (uint64_t) mult20(ip, qp));
}

// the rest of GPS_Method (:222-449); writes SET_CG_NCO; -> Inav
KG_TRK_FN uint32_t service_cg(chan &c)
{
    const uint32_t inav = (c.ser[0] >> (INTEG_BITS - 1)) & 1;
    const uint64_t pp = (uint64_t) mult20(c.ser[1], c.ser[1]) + (uint64_t) mult20(c.ser[0], c.ser[0]);
    const uint64_t pe = (uint64_t) mult20(c.ser[2], c.ser[2]) + (uint64_t) mult20(c.ser[3], c.ser[3]);
    const uint64_t pl = (uint64_t) mult20(c.ser[4], c.ser[4]) + (uint64_t) mult20(c.ser[5], c.ser[5]);
    c.fw.iq[2] = (uint32_t) pe; c.fw.iq[3] = (uint32_t) (pe >> 32);
    c.fw.iq[4] = (uint32_t) pl; c.fw.iq[5] = (uint32_t) (pl >> 32);
    c.fw.unlocked = (uint16_t) ((((pp - pe) >> 63) | ((pp - pl) >> 63)) << 15);
    uint64_t err = pe - pl;
    if (c.fw.e1b_mode && c.fw.lo_polarity) {
        const uint64_t aacf = ((int64_t) err < 0) ? (uint64_t) 0 - err : err;
        err = (c.fw.lo_polarity == 1) ? err + aacf : err - aacf;
    }
    if (c.loop_on) c.cg_rate = close_loop(&c.fw.cg_freq, c.fw.cg_gain, err);
    bool save = c.fw.e1b_mode != 0;
    if (!save) {
        if (inav != c.fw.nav_prev) {
            c.fw.nav_prev = (uint16_t) inav;
            if (c.fw.nav_ms != 0) c.fw.nav_glitch++;
            c.fw.nav_ms = 1;
        } else if (c.fw.nav_ms != 19) {
            c.fw.nav_ms++;
        } else {
            save = true;
        }
    }
    if (save) {
        c.fw.nav_ms = 0;
        const uint32_t cnt = c.fw.nav_bits;
        c.fw.nav_bits = (uint16_t) ((cnt + 1) & (MAX_NAV_BITS - 1));
        uint16_t *w = &c.fw.nav_buf[(cnt >> 4) & (MAX_NAV_BITS / 16 - 1)];
        *w = (uint16_t) ((*w << 1) + inav);
    }
    return inav;
}

// what a segment of edges with constant rates starts from
struct seg {
    uint64_t p0;                          // cg_phase
    uint32_t r, psi0, lr, n0, len_code, e1b, frozen;
    uint32_t p_old, l_old, lat_old;       // the latches before edge 0
    uint32_t e_new, p_new, l_new;         // frozen: E, P, L from edge 1 on
    uint32_t e_old;                       // frozen: E before edge 0
};

KG_TRK_FN uint32_t tab_bit(const uint32_t *tab, uint32_t i) { return (tab[i >> 5] >> (i & 31)) & 1; }

// E1B: E before the edge that crosses quarter boundary x + 1 of a running segment: chip x >> 2 (the latch still holds its old value
// in chip 0), BOC bit (x >> 1) & 1
KG_TRK_FN uint32_t e1b_e_at_quarter(const seg &s, const uint32_t *tab, uint32_t x)
{
    const uint32_t chip = x >> 2;
    return (chip ? tab_bit(tab, (s.n0 + chip) % s.len_code) : s.lat_old) ^ ((x >> 1) & 1);
}

// E, P, L before edge k of a running segment (bits 0, 1, 2); *chips_nchip: the generator's nchip and the `chips` register there
KG_TRK_FN uint32_t epl_at(const seg &s, const uint32_t *tab, uint32_t k, uint32_t *nchip, uint32_t *chips, uint32_t chips_old, uint32_t *lat)
{
    const uint64_t a = s.p0 + (uint64_t) k * s.r;
    const uint32_t fc = (uint32_t) (a >> 32);
    const uint32_t n = (s.n0 + fc) % s.len_code;
    uint32_t e, p = s.p_old, l = s.l_old, ch = chips_old, la = s.lat_old;
    if (!s.e1b) {
        const uint32_t h = (uint32_t) (a >> 31), h0 = (uint32_t) (s.p0 >> 31);
        e = tab_bit(tab, n);
        if (h >= 1) {
            const uint32_t m = (h - 1) | 1;                     // the last odd multiple of 2^31 at or below A(k)
            if (m > h0) {
                const uint32_t cc = (s.n0 + (m >> 1)) % s.len_code;
                p = tab_bit(tab, cc);
                ch = cc;
            }
        }
        if (fc >= 1) {
            const uint32_t m = 2 * fc - 1;                      // P at that carry: latched at the middle of chip fc - 1, if within the segment
            l = (m > h0) ? tab_bit(tab, (s.n0 + fc - 1) % s.len_code) : s.p_old;
        }
    } else {
        const uint32_t q = (uint32_t) (a >> 30), q0 = (uint32_t) (s.p0 >> 30);
        if (fc >= 1) la = tab_bit(tab, n);
        e = la ^ ((uint32_t) (a >> 31) & 1);
        if (q >= 1) {
            const uint32_t m = (q - 1) | 1;                     // last odd boundary
            if (m > q0) p = e1b_e_at_quarter(s, tab, m - 1);
        }
        if (q >= 2) {
            const uint32_t m = q & ~1u;                         // last even boundary
            if (m > q0) {
                l = (m - 1 > q0) ? e1b_e_at_quarter(s, tab, m - 2) : s.p_old;
                const uint32_t mh = ((q - 2) & ~3u) + 2;        // last boundary that is 2 mod 4
                if (mh > q0) ch = (s.n0 + (mh >> 2)) % s.len_code;
            }
        }
    }
    if (nchip) { *nchip = n; *chips = ch; *lat = la; }
    return e | (p << 1) | (l << 2);
}

// 64 edges (cnt <= 64 of them) from edge k0 of a segment: the six mixer outputs of every edge, as words (order ip qp ie qe il ql).
// A running segment's word starts from the closed form at edge k0 and then follows the phase edge by edge: the carries are read off
// the phase (r < 2^29: at most one multiple of 2^30 per edge) and latch as demod.v:154-194 says.
KG_TRK_FN void mix_word(const seg &s, const uint32_t *tab, uint32_t k0, uint32_t cnt, uint64_t samp, uint64_t m[6])
{
    uint64_t we = 0, wp = 0, wl = 0, wi = 0, wq = 0;
    uint32_t psi = s.psi0 + k0 * s.lr;
    if (s.frozen) {
        const uint64_t all = ~(uint64_t) 0, first = k0 == 0 ? 1 : 0;        // edge 0 still sees the old latches
        we = (s.e_new ? all & ~first : 0) | (s.e_old ? first : 0);
        wp = (s.p_new ? all & ~first : 0) | (s.p_old ? first : 0);
        wl = (s.l_new ? all & ~first : 0) | (s.l_old ? first : 0);
    } else {
        uint32_t n, chips, lat;
        const uint32_t epl = epl_at(s, tab, k0, &n, &chips, 0, &lat);
        uint32_t e = epl & 1, p = (epl >> 1) & 1, l = epl >> 2;
        uint32_t ph = (uint32_t) (s.p0 + (uint64_t) k0 * s.r);
        for (uint32_t i = 0; i < cnt; i++) {
            if (s.e1b) e = lat ^ (ph >> 31);
            we |= (uint64_t) e << i; wp |= (uint64_t) p << i; wl |= (uint64_t) l << i;
            const uint32_t nx = ph + s.r;
            if ((nx ^ ph) >> 30) {                                          // quarter_chip
                const bool full = nx < ph, half = full || ((nx ^ ph) >> 31);
                if (full) {
                    l = p;
                    n = n + 1 == s.len_code ? 0 : n + 1;
                    if (s.e1b) lat = tab_bit(tab, n); else e = tab_bit(tab, n);
                } else if (half) {
                    if (s.e1b) l = p; else p = e;
                } else if (s.e1b) {
                    p = e;
                }
            }
            ph = nx;
        }
    }
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t top = psi >> 30;
        wi |= (uint64_t) ((0xCu >> top) & 1) << i;              // lo_sin = 4'b1100
        wq |= (uint64_t) ((0x6u >> top) & 1) << i;              // lo_cos = 4'b0110
        psi += s.lr;
    }
    const uint64_t keep = cnt >= 64 ? ~(uint64_t) 0 : (((uint64_t) 1 << cnt) - 1);
    m[0] = (samp ^ wp ^ wi) & keep; m[1] = (samp ^ wp ^ wq) & keep;
    m[2] = (samp ^ we ^ wi) & keep; m[3] = (samp ^ we ^ wq) & keep;
    m[4] = (samp ^ wl ^ wi) & keep; m[5] = (samp ^ wl ^ wq) & keep;
}

// 64 sample bits from bit `bit` of a packed stream (LSB first, sampler.v) of `nbytes` bytes: no byte beyond them is read
KG_TRK_FN uint64_t sample_word(const uint8_t *bits, uint64_t nbytes, uint64_t bit)
{
    const uint64_t b0 = bit >> 3;
    const unsigned sh = (unsigned) (bit & 7);
    uint64_t lo = 0;
    uint32_t hi = 0;
    for (unsigned i = 0; i < 8; i++)
        if (b0 + i < nbytes) lo |= (uint64_t) bits[b0 + i] << (8 * i);
    if (sh && b0 + 8 < nbytes) hi = bits[b0 + 8];
    return sh ? (lo >> sh) | ((uint64_t) hi << (64 - sh)) : lo;
}

KG_TRK_FN uint32_t replica(const chan &c)                       // demod.v:290-292
{
    return ((~c.cg_phase >> 31) << 17) | (((c.cg_phase >> 26) & 31) << 12) | ((c.chips & 0x3FF) << 2) | ((c.chips >> 10) & 3);
}

KG_TRK_FN uint32_t popc64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t) __popcll(v);
#else
    return (uint32_t) __builtin_popcountll(v);
#endif
}

// The sums of one segment over the lanes that share it: host code is one lane.
struct seg_sums { uint32_t cnt[6]; uint32_t last; };            // last: the six mixer outputs of the segment's last edge

KG_TRK_FN seg_sums seg_lane(const seg &s, const uint32_t *tab, const uint8_t *bits, uint64_t nbytes, uint64_t bit0, uint32_t len,
                            uint32_t lane, uint32_t nlanes)
{
    seg_sums o = {{0, 0, 0, 0, 0, 0}, 0};
    for (uint32_t k0 = lane * 64; k0 < len; k0 += nlanes * 64) {
        const uint32_t cnt = len - k0 < 64 ? len - k0 : 64;
        uint64_t m[6];
        mix_word(s, tab, k0, cnt, sample_word(bits, nbytes, bit0 + k0), m);
        for (int i = 0; i < 6; i++) o.cnt[i] += popc64(m[i]);
        if (k0 + cnt == len)
            for (int i = 0; i < 6; i++) o.last |= (uint32_t) ((m[i] >> (cnt - 1)) & 1) << i;
    }
    return o;
}

// the first edge (counted from the segment's start) that sets ms0: the middle of the chip at which nchip is 0 (C/A: (2 c + 1) 2^31;
// E1B: (4 c + 2) 2^30, the same number)
KG_TRK_FN uint64_t next_ms0_edge(uint32_t p0, uint32_t r, uint32_t n0, uint32_t len_code)
{
    uint64_t c = (len_code - n0) % len_code;
    uint64_t m = (2 * c + 1) << 31;
    if (m <= p0) m = (2 * (uint64_t) len_code + 1) << 31;       // only for c = 0: this chip's middle has passed
    return (m - p0 + r - 1) / r - 1;
}

// The control of one channel over `nclocks` edges: every lane of a wave runs it with the same values, the segments' sums are
// the only thing shared out (REDUCE adds a seg_sums over the lanes; the host's is the identity).  Lane 0's `c`, `out` and
// `*count` are the result.  cg_cnt: gps.v's pause counter before edge 0 (one for the bank; the caller advances it).
template <class Reduce>
KG_TRK_FN void run(chan &c, const uint32_t *tab, const uint8_t *bits, uint64_t nbytes, uint64_t bit0, uint64_t nclocks, uint64_t clock0,
                   uint32_t cg_cnt, epoch *out, int cap, int *count, uint32_t lane, uint32_t nlanes, Reduce reduce)
{
    const uint32_t e1b = (c.sat & E1B_MODE) != 0, len_code = e1b ? E1B_CODELEN : L1_CODELEN;
    const uint32_t mask = (1u << INTEG_BITS) - 1;
    uint64_t t = 0;
    int n = 0;
    while (t < nclocks) {
        if (c.fault || c.cg_rate < (1u << 27) || c.cg_rate >= (1u << 29)) { c.fault = 1; break; }
        if (c.ms1_due == 0) {                                   // this edge sees ms1: ser_iq latches, the filters restart, lsb <- 0
            for (int i = 0; i < 6; i++) { c.ser[i] = c.integ[i]; c.integ[i] = (c.lsb - 1) & mask; }
            c.lsb = 1;                                          // (the edge below then adds the old lsb, and the ones after it 0 1 0 1 ...)
            c.ms1_clock = clock0 + t;
            c.ms1_due = -1;
        }
        uint64_t len = nclocks - t;
        if (c.ms1_due > 0 && (uint64_t) c.ms1_due < len) len = c.ms1_due;
        if (c.lo_due > 0 && (uint64_t) c.lo_due < len) len = c.lo_due;
        if (c.cg_due > 0 && (uint64_t) c.cg_due < len) len = c.cg_due;
        seg s;
        s.p0 = c.cg_phase; s.r = c.cg_rate; s.psi0 = c.lo_phase; s.lr = c.lo_rate; s.n0 = c.nchip; s.len_code = len_code; s.e1b = e1b;
        s.p_old = c.cg_p; s.l_old = c.cg_l; s.lat_old = c.lat; s.frozen = !c.cg_en;
        s.e_old = s.e_new = s.p_new = s.l_new = 0;
        bool fires = false;
        if (s.frozen) {
            const uint64_t left = (uint64_t) ((cg_cnt - (uint32_t) t) & 0xFFFF) + 1;      // through the edge at which cg_cnt is 0
            if (left < len) len = left;
            const uint64_t a = s.p0 + s.r;
            const bool full = (a >> 32) != 0, half = full || ((a >> 31) != (s.p0 >> 31)), quarter = half || ((a >> 30) != (s.p0 >> 30));
            uint32_t lat_new = c.lat;
            s.p_new = c.cg_p; s.l_new = c.cg_l;
            if (!e1b) {
                s.e_old = s.e_new = tab_bit(tab, c.nchip);
                if (half && full) s.l_new = c.cg_p;
                if (half && !full) { s.p_new = s.e_old; c.chips = c.nchip; }
            } else {
                s.e_old = c.lat ^ (c.cg_phase >> 31);
                if (full) { lat_new = tab_bit(tab, c.nchip); s.l_new = c.cg_p; }
                if (quarter && !full) {
                    if (half) { s.l_new = c.cg_p; c.chips = c.nchip; }
                    else s.p_new = s.e_old;
                }
                s.e_new = lat_new ^ (c.cg_phase >> 31);
            }
            c.lat = lat_new;
        } else {
            const uint64_t j0 = next_ms0_edge(c.cg_phase, c.cg_rate, c.nchip, len_code);
            if (j0 + 1 <= len) { len = j0 + 1; fires = true; }
        }
        const seg_sums sums = reduce(seg_lane(s, tab, bits, nbytes, bit0 + t, (uint32_t) len, lane, nlanes));
        const uint32_t ones = (uint32_t) (c.lsb ? (len + 1) / 2 : len / 2);
        for (int i = 0; i < 6; i++) {
            const uint32_t dsum = ((c.d >> i) & 1) + sums.cnt[i] - ((sums.last >> i) & 1);
            c.integ[i] = (c.integ[i] + ones - dsum) & mask;
        }
        c.d = sums.last;
        c.lsb ^= (uint32_t) (len & 1);
        c.lo_phase += (uint32_t) len * c.lo_rate;
        if (s.frozen) {
            c.cg_p = s.p_new; c.cg_l = s.l_new;
            if (((cg_cnt - (uint32_t) t) & 0xFFFF) + 1 == len) c.cg_en = 1;
        } else {
            uint32_t nch, chips, lat;
            const uint32_t epl = epl_at(s, tab, (uint32_t) len, &nch, &chips, c.chips, &lat);
            c.cg_p = (epl >> 1) & 1; c.cg_l = epl >> 2;
            c.nchip = nch; c.chips = chips; c.lat = lat;
            c.cg_phase = (uint32_t) (s.p0 + len * s.r);
        }
        t += len;
        if (c.ms1_due > 0) c.ms1_due -= (int32_t) len;
        if (c.lo_due > 0 && (c.lo_due -= (int32_t) len) == 0) { service_lo(c); c.lo_due = -1; }
        if (c.cg_due > 0 && (c.cg_due -= (int32_t) len) == 0) {
            const uint32_t inav = service_cg(c);
            c.cg_due = -1;
            if (n < cap && lane == 0) {
                epoch e;
                e.clock = c.ms1_clock;
                e.ip = sext20(c.ser[0]); e.qp = sext20(c.ser[1]); e.ie = sext20(c.ser[2]);
                e.qe = sext20(c.ser[3]); e.il = sext20(c.ser[4]); e.ql = sext20(c.ser[5]);
                e.lo_rate = c.lo_rate; e.cg_rate = c.cg_rate;
                e.flags = (c.fw.unlocked ? 1u : 0u) | (inav << 1);
                e.pad_ = 0;
                out[n] = e;
            }
            if (n < cap) n++;
        }
        if (fires) { c.ms1_due = 1; c.lo_due = (int32_t) c.lo_delay; c.cg_due = (int32_t) c.cg_delay; }
    }
    *count = c.fault ? -1 - n : n;                              // a stopped channel says so where the caller reads its count
}

// cacode.v: G1 / G2 from the seed `rst` loads, 1023 chips through the taps or, under g2_init, g1[10] ^ g2[10]
KG_TRK_FN void ca_table(uint32_t sat, chan_tab *out)
{
    const uint32_t g2_init = sat & G2_INIT, init = sat & 0x3FF, t0 = (init >> 4) & 15, t1 = init & 15;
    uint32_t g1 = 0x3FF, g2 = g2_init ? init : 0x3FF;                   // bit i - 1 = stage i
    for (int i = 0; i < TABLE_WORDS; i++) out->w[i] = 0;
    for (int n = 0; n < L1_CODELEN; n++) {
        const uint32_t chip = g2_init ? ((g1 >> 9) ^ (g2 >> 9)) & 1 : ((g1 >> 9) ^ (g2 >> (t0 - 1)) ^ (g2 >> (t1 - 1))) & 1;
        out->w[n >> 5] |= chip << (n & 31);
        const uint32_t f1 = ((g1 >> 2) ^ (g1 >> 9)) & 1;
        const uint32_t f2 = ((g2 >> 1) ^ (g2 >> 2) ^ (g2 >> 5) ^ (g2 >> 7) ^ (g2 >> 8) ^ (g2 >> 9)) & 1;
        g1 = ((g1 << 1) | f1) & 0x3FF;
        g2 = ((g2 << 1) | f2) & 0x3FF;
    }
}

// would the held chip events of a paused channel keep ms0 set?
KG_TRK_FN bool holds_ms0(const chan &c)
{
    if (c.cg_en || c.nchip != 0) return false;
    if (c.cg_due > 0) return true;                                      // the word still to be written decides: not known here
    const uint64_t a = (uint64_t) c.cg_phase + c.cg_rate;
    return (a >> 32) == 0 && (a >> 31) != (c.cg_phase >> 31);          // half_chip && !full_chip (E1B: && quarter_chip, implied)
}


// The commands that can bring that state about, tried on a copy: a command that would is refused with nothing changed.
KG_TRK_FN bool pause_would_hold_ms0(chan c) { c.cg_en = 0; return holds_ms0(c); }
KG_TRK_FN bool rate_would_hold_ms0(chan c, uint32_t rate) { c.cg_rate = rate; return holds_ms0(c); }
KG_TRK_FN bool reset_would_hold_ms0(chan c) { c.cg_phase = 0; c.nchip = 0; return holds_ms0(c); }

}  // namespace kg_trk_cf
