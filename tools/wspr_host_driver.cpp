// csrc/kg_wspr.h on the host: the twin the WSPR kernels are held to, behind the script loop and records of tools/ref/wspr_harness.h, so
// that tests/test_wspr_cpu.py can compare it with tests/golden/wspr_ref.npz (made from the reference's own statements) record by record.
// The schedule is kg_wspr.h's sched_block, the ops are carried out as the kernels do, with wspr_dft512 (the golden's stand-in for FFTW)
// as the transform: with the same transform every row, plane, peak and candidate is the reference's bit for bit.
// Built with g++ -O2 -ffp-contract=off.  A cycle end's cond[2], cond[3]: 1 if every candidate's winning sync1 is strictly above its
// runner-up, and the bits of the least (winner - runner-up) / winner over the candidates (the golden's maker records both).
#include "../flydog_sdr_gps_amd/csrc/kg_wspr.h"

using namespace kg_wspr_cf;

#include "ref/wspr_harness.h"

static state_t st;
static float idat[2][TPOINTS], qdat[2][TPOINTS], pwr_samp[2][NFFT][NT], pwr_sampavg[2][NFFT], savg[NFFT], win[NFFT];

static void flush_events(const sched_t &sp, size_t from)
{
    for (size_t k = from; k < sp.evs.size(); k++)
        if (sp.evs[k].kind == EV_STATUS) rec_status(sp.evs[k].a);
}

static void do_cycle(int half)
{
    cycle_t cy;
    cycle_end(&pwr_samp[half][0][0], pwr_sampavg[half], st.wspr_type, st.more_candidates, cy);
    // the runner-up of every candidate, by the search run again
    static const unsigned char pr3[NSYM] = KG_WSPR_PR3;
    float sm[NBINS];
    pk_t pk[MAX_NPK];
    cand_t c0[MAX_NPK];
    renormalize(pwr_sampavg[half], st.wspr_type, sm);
    const int npk = peak_list(sm, st.more_candidates, min_snr_value(), snr_scaling(st.wspr_type), pk, c0);
    int32_t cond[4] = {0, 0, 1, 0};
    float least = INFINITY;
    for (int pki = 0; pki < npk; pki++) {
        const int if0 = if0_of(c0[pki].freq0);
        auto rt = [&](int bin, int kindex) { const float p = KG_WSPR_SQRT(pwr_samp[half][bin][kindex]); return p; };
        float a = -INFINITY, b = -INFINITY;
        for (int h = 0; h < NHYP; h++) {
            int ifr, k0, idrift;
            hyp_of(h, if0, &ifr, &k0, &idrift);
            const float s = sync_of(rt, [&](int k) { return ifd_of(ifr, k, idrift); }, pr3, k0);
            if (s > a) { b = a; a = s; } else if (s > b) b = s;
        }
        if (a > -INFINITY) {
            if (!(a > b)) cond[2] = 0;
            const float rel = (a - b) / a;
            if (rel < least) least = rel;
        }
    }
    cond[3] = bits_of(least);
    rec_pk rp[MAX_NPK];
    rec_cand rc[MAX_NPK];
    for (int r = 0; r < cy.npk; r++) {
        rp[r] = rec_pk{cy.pk[r].bin0, cy.pk[r].freq0, cy.pk[r].snr0};
        rc[r] = rec_cand{cy.cand[r].freq0, cy.cand[r].shift0, cy.cand[r].drift0, cy.cand[r].sync0, cy.cand[r].freq_idx, cy.cand[r].bin0};
    }
    rec_cycle(half, cy.npk, rp, rc, cond);
}

static void do_group(int half, int grp, int flag)
{
    float in[NFFT][2], out[NFFT][2];
    memset(savg, 0, sizeof savg);
    for (int i = grp * FPG; i < grp * FPG + FPG; i++) {
        for (int j = 0; j < NFFT; j++) {
            const int k = i * HSPS + j;
            in[j][0] = windowed(idat[half][k], win[j]);
            in[j][1] = windowed(qdat[half][k], win[j]);
        }
        wspr_dft512(in, out);
        for (int j = 0; j < NFFT; j++) {
            const int k = unwrap(j);
            const float pwr = power(out[k][0], out[k][1]);
            pwr_samp[half][j][i] = pwr;
            pwr_sampavg[half][j] += pwr;
            savg[j] += pwr;
        }
    }
    unsigned char ws[NBINS + 1];
    row_of(savg, st.wspr_type, flag, ws);
    rec_row(grp, half, savg, ws);
}

static int h_init(double snd_rate)
{
    if (cmd_init(st, snd_rate)) return 11;
    for (int i = 0; i < NFFT; i++) win[i] = window_at(i);
    rec_status(ST_IDLE);
    return 0;
}
static int h_capture(int on)
{
    if (!st.inited) return 14;
    sched_t sp;
    cmd_capture(st, on, &sp);
    flush_events(sp, 0);
    return 0;
}
static int h_type(int type)
{
    if (!st.inited) return 14;
    return cmd_type(st, type) ? 12 : 0;
}
static int h_more(int on)
{
    if (!st.inited) return 14;
    st.more_candidates = on != 0;
    return 0;
}
static int h_block(const float *iq, int n, int min, int sec)
{
    if (!st.inited) return 14;
    if (!time_ok(min, sec)) return 13;
    sched_t sp;
    sched_block(st, sp, 0, 0, n, min, sec);
    // the events in the order the reference sends them: a status change ahead of the block's first op, then per cycle end DECODING, peaks, resume
    size_t ev = 0;
    if (!sp.evs.empty() && sp.evs[0].kind == EV_STATUS && sp.evs[0].b == ST_RUNNING) { rec_status(sp.evs[0].a); ev++; }      // the sync of :644
    for (const op_t &o : sp.ops) {
        if (o.kind == OP_COPY)
            for (int t = 0; t < o.n; t++) {
                idat[o.half][o.a + t] = iq[2 * (o.src + (int64_t) t * st.int_decimate)];
                qdat[o.half][o.a + t] = iq[2 * (o.src + (int64_t) t * st.int_decimate) + 1];
            }
        else if (o.kind == OP_ZERO) memset(pwr_sampavg[o.half], 0, sizeof pwr_sampavg[o.half]);
        else {
            do_group(o.half, o.a, o.b);
            if (o.a == LAST_GROUP) {
                if (!(ev + 2 < sp.evs.size() && sp.evs[ev].a == ST_DECODING && sp.evs[ev + 1].kind == EV_PEAKS)) return 20;
                rec_status(sp.evs[ev].a);
                do_cycle(sp.evs[ev + 1].a);
                rec_status(sp.evs[ev + 2].a);
                ev += 3;
            }
        }
    }
    return ev == sp.evs.size() ? 0 : 21;
}
static int h_load(const float *ps, const float *pa)
{
    if (!st.inited) return 14;
    memcpy(pwr_samp[0], ps, sizeof pwr_samp[0]);
    memcpy(pwr_sampavg[0], pa, sizeof pwr_sampavg[0]);
    st.decode_ping_pong = 0;
    do_cycle(0);
    return 0;
}
static void h_dump(int32_t *o, FILE *planes)
{
    const int32_t v[18] = {st.inited, st.capture, st.reset, st.tsync, st.ping_pong, st.fft_ping_pong, st.decode_ping_pong, st.decim, st.didx, st.group,
                           st.status, st.status_resume, st.inited ? st.last_sec : -1, st.abort_decode, st.inited ? st.wspr_type : TYPE_2MIN, st.more_candidates,
                           st.int_decimate, st.cycles};
    memcpy(o, v, sizeof v);
    fwrite(pwr_sampavg, sizeof pwr_sampavg, 1, planes);
    fwrite(pwr_samp, sizeof pwr_samp, 1, planes);
    fwrite(idat, sizeof idat, 1, planes);
    fwrite(qdat, sizeof qdat, 1, planes);
}
