// kg_nav.h -- the arithmetic of nav frame sync: what CHANNEL::Tracking() does with the nav bits (gps/channel.cpp:441-506, the
// `holding` loop; ParityCheck :731-832; L1_parity :125-135) and, for Galileo, E1B_subframe (gps/GNSS-SDRLIB/sdrnav_gal.cpp:382-514:
// the 30 x 8 de-interleave, KA9Q's K = 7 rate-1/2 decoder gps/ka9q-fec/viterbi27_port.cpp with polynomials 0x4f / 0x6d, the
// even/odd test, checkcrc_e1b :293-319, the alert bits, decode_word5's health bits :162-174), for the device (kg_nav.hip) and,
// compiled by a host compiler, for tools/nav_host_driver.cpp -- as kg_trk.h is.  All of it is integer arithmetic.
//
// Bits are held packed, the first bit of the stream highest: bit i of a window is bit 31 - (i & 31) of word i >> 5.  A window is
// the held tail of a channel followed by the newly pushed bits; two words beyond its last bit are readable.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KG_NAV_FN __host__ __device__ static inline
#else
#define KG_NAV_FN static inline
#endif

namespace kg_nav_cf {

enum { MODE_L1 = 0, MODE_E1B = 1, L1_BITS = 300, E1B_BITS = 500, E1B_HALF = 250, HELD_WORDS = 16,
       L1_PRE_UP = 0x8B, L1_PRE_INV = 0x74,             // L1preambleUpright / Inverse, channel.cpp:122-123
       E1B_PRE_UP = 0x160, E1B_PRE_INV = 0x29F,         // E1BpreambleUpright / Inverse, channel.cpp:144-145
       ERR_SLIP = 1, ERR_CRC = 2, ERR_ALERT = 3, ERR_OOS = 4, ERR_PAGE = 5,     // gps/gps.h:187-191
       ERR_PARITY = 16 };

struct chan {
    uint64_t base, pushed;                // the stream index of buf[0]; bits pushed since set_mode
    int32_t mode, holding;
    int32_t wlen, nnew;                   // of the push in flight: the window's length, the bits it adds
    uint32_t nav_ms, nav_prev, nav_glitch, pad_;
    uint32_t held[HELD_WORDS];            // buf[0 .. holding), zero beyond
};

struct res {                              // stage 1's answer for one matched head
    int32_t code, id;                     // C/A: 0x100 | inverted << 7 | first failing word (10: none).  E1B: 0x100 | inverted << 7 | err
    uint64_t w[4];                        // E1B: dec_e1b1 (120 bits from bit 63 of w[0] down), dec_e1b2 (w[2], w[3])
};

struct frame {                            // == kg_nav_frame (include/kiwigpu.h)
    uint64_t bit;
    int32_t err, consumed, inverted, id;
    uint8_t data[40];
};

KG_NAV_FN uint32_t par32(uint32_t v) { return (uint32_t) __builtin_popcount(v) & 1u; }
KG_NAV_FN uint32_t ctz64(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }

// len (1..32) bits from bit p of a window; reads words p >> 5 and (p >> 5) + 1
KG_NAV_FN uint32_t win_get(const uint32_t *win, uint32_t p, uint32_t len)
{
    const uint64_t v = ((uint64_t) win[p >> 5] << 32) | win[(p >> 5) + 1];
    return (uint32_t) (v >> (64 - len - (p & 31))) & (len == 32 ? ~0u : ((1u << len) - 1));
}

// ---- L1 C/A: IS-GPS-200 parity as L1_parity writes it.  A word is 30 bits, d1 highest; its data bits as bit 24 - i of a 24-bit value.
#define KG_NAV_D(i) (1u << (24 - (i)))
enum : uint32_t {
    L1_M0 = KG_NAV_D(1) | KG_NAV_D(2) | KG_NAV_D(3) | KG_NAV_D(5) | KG_NAV_D(6) | KG_NAV_D(10) | KG_NAV_D(11) | KG_NAV_D(12) | KG_NAV_D(13) |
            KG_NAV_D(14) | KG_NAV_D(17) | KG_NAV_D(18) | KG_NAV_D(20) | KG_NAV_D(23),                                          // ^ D29
    L1_M1 = KG_NAV_D(2) | KG_NAV_D(3) | KG_NAV_D(4) | KG_NAV_D(6) | KG_NAV_D(7) | KG_NAV_D(11) | KG_NAV_D(12) | KG_NAV_D(13) | KG_NAV_D(14) |
            KG_NAV_D(15) | KG_NAV_D(18) | KG_NAV_D(19) | KG_NAV_D(21) | KG_NAV_D(24),                                          // ^ D30
    L1_M2 = KG_NAV_D(1) | KG_NAV_D(3) | KG_NAV_D(4) | KG_NAV_D(5) | KG_NAV_D(7) | KG_NAV_D(8) | KG_NAV_D(12) | KG_NAV_D(13) | KG_NAV_D(14) |
            KG_NAV_D(15) | KG_NAV_D(16) | KG_NAV_D(19) | KG_NAV_D(20) | KG_NAV_D(22),                                          // ^ D29
    L1_M3 = KG_NAV_D(2) | KG_NAV_D(4) | KG_NAV_D(5) | KG_NAV_D(6) | KG_NAV_D(8) | KG_NAV_D(9) | KG_NAV_D(13) | KG_NAV_D(14) | KG_NAV_D(15) |
            KG_NAV_D(16) | KG_NAV_D(17) | KG_NAV_D(20) | KG_NAV_D(21) | KG_NAV_D(23),                                          // ^ D30
    L1_M4 = KG_NAV_D(1) | KG_NAV_D(3) | KG_NAV_D(5) | KG_NAV_D(6) | KG_NAV_D(7) | KG_NAV_D(9) | KG_NAV_D(10) | KG_NAV_D(14) | KG_NAV_D(15) |
            KG_NAV_D(16) | KG_NAV_D(17) | KG_NAV_D(18) | KG_NAV_D(21) | KG_NAV_D(22) | KG_NAV_D(24),                           // ^ D30
    L1_M5 = KG_NAV_D(3) | KG_NAV_D(5) | KG_NAV_D(6) | KG_NAV_D(8) | KG_NAV_D(9) | KG_NAV_D(10) | KG_NAV_D(11) | KG_NAV_D(13) | KG_NAV_D(15) |
            KG_NAV_D(19) | KG_NAV_D(22) | KG_NAV_D(23) | KG_NAV_D(24)                                                          // ^ D29
};

// one word as received -> the word as buf holds it after L1_parity (data ^= D30, parity as received); *p6: the parity computed, p[0] highest
KG_NAV_FN uint32_t l1_word(uint32_t w, uint32_t d29, uint32_t d30, uint32_t *p6)
{
    const uint32_t d = ((w >> 6) ^ (d30 ? 0xFFFFFFu : 0u)) & 0xFFFFFFu;
    *p6 = ((d29 ^ par32(d & L1_M0)) << 5) | ((d30 ^ par32(d & L1_M1)) << 4) | ((d29 ^ par32(d & L1_M2)) << 3) |
          ((d30 ^ par32(d & L1_M3)) << 2) | ((d30 ^ par32(d & L1_M4)) << 1) | (d29 ^ par32(d & L1_M5));
    return (d << 6) | (w & 63);
}

// ParityCheck's C/A arm on the head at bit p: 0 = no preamble (drop 1 bit), else 0x100 | inverted << 7 | first failing word (10: none)
KG_NAV_FN uint32_t l1_judge(const uint32_t *win, uint32_t p)
{
    const uint32_t pre = win_get(win, p, 8);
    uint32_t inv;
    if (pre == L1_PRE_UP) inv = 0;
    else if (pre == L1_PRE_INV) inv = 1;
    else return 0;
    uint32_t d29 = inv, d30 = inv;                      // p[4] = p[5] = 0 / 1
    for (uint32_t i = 0; i < 10; i++) {
        const uint32_t w = win_get(win, p + 30 * i, 30);
        uint32_t p6;
        (void) l1_word(w, d29, d30, &p6);
        if (p6 != (w & 63)) return 0x100 | (inv << 7) | i;
        d29 = (p6 >> 1) & 1; d30 = p6 & 1;
    }
    return 0x100 | (inv << 7) | 10;
}

// ---- E1B
// the preamble pair of ParityCheck's E1B arm: 0 none, 1 upright, 2 inverse
KG_NAV_FN uint32_t e1b_pre(const uint32_t *win, uint32_t p)
{
    const uint32_t a = win_get(win, p, 10), b = win_get(win, p + E1B_HALF, 10);
    if (a == E1B_PRE_UP && b == E1B_PRE_UP) return 1;
    if (a == E1B_PRE_INV && b == E1B_PRE_INV) return 2;
    return 0;
}

// enc_e1b[i] / 255 of the page half whose first symbol is window bit q: the polarity map (0 -> +1, 1 -> -1, times nav.polarity),
// interleave(.., 30, 8, ..) (out[r * 8 + c] = in[c * 30 + r]) and "+1 -> 0, -1 -> 255" with every odd symbol inverted
KG_NAV_FN uint32_t e1b_enc(const uint32_t *win, uint32_t q, uint32_t i, uint32_t inv)
{
    const uint32_t r = i >> 3, c = i & 7;
    return win_get(win, q + c * 30 + r, 1) ^ inv ^ (i & 1);
}

// Branchtab27[k].c[i] of set_viterbi27_polynomial_port({0x4f, 0x6d})
KG_NAV_FN uint32_t v27_branch(uint32_t poly, uint32_t i) { return par32((2 * i) & poly) ? 255u : 0u; }

// BFLY's half for new state s: the old metrics of states s >> 1 and (s >> 1) + 32, the two symbols (0 / 255) -> the new metric of s
KG_NAV_FN uint32_t v27_step(uint32_t s, uint32_t old_lo, uint32_t old_hi, uint32_t sym0, uint32_t sym1, uint32_t *decision)
{
    const uint32_t i = s >> 1;
    const uint32_t metric = (v27_branch(0x4f, i) ^ sym0) + (v27_branch(0x6d, i) ^ sym1);
    uint32_t m0 = old_lo + metric, m1 = old_hi + (510 - metric);
    if (s & 1) { m0 -= (metric + metric - 510); m1 += (metric + metric - 510); }
    const uint32_t d = (int32_t) (m0 - m1) > 0;
    *decision = d;
    return d ? m1 : m0;
}

// chainback_viterbi27_port(p, data, 114, 0): dec(t) is the decision word of step t (bit s: new state s).  data[15] comes back as 120
// bits, data[0]'s bit 7 = bit 63 of *o0; the 6 bits beyond the 114 are what endstate leaves there.
template <class Dec>
KG_NAV_FN void v27_chainback(Dec dec, uint64_t *o0, uint64_t *o1)
{
    uint32_t endstate = 0;
    uint64_t a = 0, b = 0;
    for (uint32_t n = 114; n-- != 0;) {
        const uint32_t k = (uint32_t) (dec(n + 6) >> (endstate >> 2)) & 1;
        endstate = (endstate >> 1) | (k << 7);
        const uint32_t byte = n >> 3, sh = 56 - 8 * (byte & 7);                        // data[n >> 3] = endstate
        if (byte < 8) a = (a & ~((uint64_t) 0xFF << sh)) | ((uint64_t) endstate << sh);
        else b = (b & ~((uint64_t) 0xFF << sh)) | ((uint64_t) endstate << sh);
    }
    *o0 = a; *o1 = b;
}

KG_NAV_FN uint32_t half_bit(uint64_t w0, uint64_t w1, uint32_t n) { return (uint32_t) (n < 64 ? w0 >> (63 - n) : w1 >> (127 - n)) & 1; }
KG_NAV_FN uint32_t half_byte(uint64_t w0, uint64_t w1, uint32_t b) { return (uint32_t) (b < 8 ? w0 >> (56 - 8 * b) : w1 >> (56 - 8 * (b - 8))) & 0xFF; }

KG_NAV_FN uint32_t crc24q_bit(uint32_t crc, uint32_t bit)           // rtkcmn.cpp's table is this polynomial a byte at a time
{
    crc ^= bit << 23;
    return ((crc << 1) ^ ((crc & 0x800000u) ? 0x1864CFBu : 0u)) & 0xFFFFFFu;
}

// E1B_subframe from "check page part (even/odd)" on, with decode_page_e1b reduced to the id and word 5's health bits -> err; *id
KG_NAV_FN int32_t e1b_page(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, int32_t *id)
{
    *id = 0;
    if (half_bit(a0, a1, 0)) return ERR_SLIP;
    const int32_t type = (int32_t) ((a0 >> 56) & 63);                                  // getbitu(dec_e1b1, 2, 6)
    uint32_t crc = 0, msg = 0;                          // checkcrc_e1b: 114 + 82 bits (the 4 right-aligning zeros leave a zero crc zero)
    for (uint32_t n = 0; n < 114; n++) crc = crc24q_bit(crc, half_bit(a0, a1, n));
    for (uint32_t n = 0; n < 82; n++) crc = crc24q_bit(crc, half_bit(b0, b1, n));
    for (uint32_t n = 82; n < 106; n++) msg = (msg << 1) | half_bit(b0, b1, n);
    if (crc != msg) { *id = type; return ERR_CRC; }
    if (half_bit(a0, a1, 1) && half_bit(b0, b1, 1)) return ERR_ALERT;
    *id = type;
    int32_t err = 0;
    if (type == 5) {                                    // decode_word5: OFFSET1 + 69 (2 bits), OFFSET1 + 72
        const uint32_t e1bhs = (half_bit(a0, a1, 71) << 1) | half_bit(a0, a1, 72);
        if (e1bhs == 1 || e1bhs == 3) err = ERR_OOS;
        if (half_bit(a0, a1, 74)) err = ERR_OOS;
    }
    return err;
}

// ---- the nav-bit machine of service_cg (kg_trk.h:103-121; kiwi.gps.asm's NavSave) on one epoch's Inav -> a bit was saved
KG_NAV_FN bool nav_bit_step(int32_t mode, uint32_t *nav_ms, uint32_t *nav_prev, uint32_t *nav_glitch, uint32_t inav)
{
    bool save = mode == MODE_E1B;
    if (!save) {
        if (inav != *nav_prev) {
            *nav_prev = inav;
            if (*nav_ms != 0) *nav_glitch = (*nav_glitch + 1) & 0xFFFF;
            *nav_ms = 1;
        } else if (*nav_ms != 19) {
            (*nav_ms)++;
        } else {
            save = true;
        }
    }
    if (save) *nav_ms = 0;
    return save;
}

// ---- stage 2: the `holding` loop over stage 1's answers.  match: bit o & 63 of word o >> 6 set = the head at o passed the preamble
// test (no bit at an offset whose frame does not fit the window); rs[o]: its answer.  Writes the records (at most cap), the tail and
// the stream index into c -> the record count.
KG_NAV_FN int32_t walk(chan &c, const uint32_t *win, const uint64_t *match, const res *rs, frame *out, int32_t cap)
{
    const int32_t sub = c.mode == MODE_E1B ? E1B_BITS : L1_BITS, W = c.wlen;
    int32_t pos = 0, n = 0;
    if (W >= sub) {
        const int32_t last = W - sub;
        while (pos <= last) {
            uint32_t wi = (uint32_t) pos >> 6;
            uint64_t m = match[wi] & (~(uint64_t) 0 << (pos & 63));
            while (!m && (int32_t) ((wi + 1) << 6) <= last) m = match[++wi];
            if (!m) { pos = last + 1; break; }                                          // every head left dropped one bit
            pos = (int32_t) ((wi << 6) + ctz64(m));
            if (pos > last) { pos = last + 1; break; }
            const res r = rs[pos];
            const int32_t inv = (r.code >> 7) & 1, low = r.code & 0x7F;
            int32_t err, id, consumed;
            if (c.mode == MODE_E1B) {
                err = low; id = r.id;
                consumed = err == ERR_SLIP ? E1B_HALF : E1B_BITS;
            } else if (low < 10) {
                err = ERR_PARITY; id = low; consumed = 30 * (low + 1);
            } else {
                err = 0; id = (int32_t) win_get(win, (uint32_t) pos + 49, 3) ^ (win_get(win, (uint32_t) pos + 29, 1) ? 7 : 0);
                consumed = L1_BITS;
            }
            if (n < cap) {
                frame *f = out + n;
                f->bit = c.base + (uint64_t) pos; f->err = err; f->consumed = consumed; f->inverted = inv; f->id = id;
                uint32_t k = 0;
                if (c.mode == MODE_E1B) {
                    for (uint32_t b = 0; b < 15; b++) f->data[k++] = (uint8_t) half_byte(r.w[0], r.w[1], b);
                    for (uint32_t b = 0; b < 15; b++) f->data[k++] = (uint8_t) half_byte(r.w[2], r.w[3], b);
                } else if (err == 0) {
                    uint64_t acc = 0;
                    uint32_t have = 0, d29 = (uint32_t) inv, d30 = (uint32_t) inv;
                    for (uint32_t i = 0; i < 10; i++) {
                        uint32_t p6;
                        acc = (acc << 30) | l1_word(win_get(win, (uint32_t) pos + 30 * i, 30), d29, d30, &p6);
                        have += 30;
                        d29 = (p6 >> 1) & 1; d30 = p6 & 1;
                        while (have >= 8) { f->data[k++] = (uint8_t) (acc >> (have - 8)); have -= 8; }
                    }
                    f->data[k++] = (uint8_t) (acc << (8 - have));                       // the last 4 bits, high in their byte
                }
                while (k < 40) f->data[k++] = 0;
            }
            n++;
            pos += consumed;
        }
    }
    const int32_t hold = W - pos;
    for (int32_t j = 0; j < HELD_WORDS; j++) {
        const int32_t left = hold - 32 * j;
        c.held[j] = left <= 0 ? 0u : win_get(win, (uint32_t) (pos + 32 * j), 32) & (left >= 32 ? ~0u : ~(~0u >> left));
    }
    c.holding = hold;
    c.base += (uint64_t) pos;
    c.pushed += (uint64_t) c.nnew;
    c.wlen = 0; c.nnew = 0;
    return n < cap ? n : cap;
}

// how many records a push of nbits new bits can give at most: a record's head is at least 30 (C/A, a parity error in word 0) or 250
// (E1B, a slip) bits behind the one before it, the first head at the window's bit 0 or later and the last at holding + nbits - sub
// or before, with holding <= sub - 1
KG_NAV_FN int64_t max_records(int32_t mode, int64_t nbits)
{
    const int64_t step = mode == MODE_E1B ? E1B_HALF : 30;
    return nbits <= 0 ? 0 : (nbits - 1) / step + 1;
}

}  // namespace kg_nav_cf
