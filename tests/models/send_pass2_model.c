/* CPU model of the two-sender wave path's token pass (pcc-rl_amd/csrc/pcc_sim.hip: heavy_mi2), with the kernel's own
 * integer / floating-point operations, against the plain merged recurrence (ns:66-84, 155-178 for two senders sharing the
 * link; events of equal time: sender 0 first).  Test infrastructure (tests/test_send_pass_model.py): a mismatch is a
 * counter-example for the pass's preconditions, found without a GPU.
 *
 *   gcc -O2 -fPIC -shared -ffp-contract=off send_pass2_model.c -o libsend_pass2_model.so -lm
 *
 * The pass covers `lanes * per_lane` merged positions (the kernel: 64 x 1); per_lane = 4 is the variant with one Philox
 * block per lane.  Whatever the token pass does not commit is sent by the plain recurrence, 64 packets at a time (the
 * kernel's accept chain / serial pass, which have no preconditions).
 *
 * Second half of the file: the two SWEEP formulations of heavy_mi2 (pcc-rl_amd/csrc/pcc_wave_pass.h) -- the 256-position sweep
 * pass, four positions per lane, and the 64-lane pass settled side by side, one position per lane -- lane by lane and sweep
 * by sweep as the kernel computes them, inside a driver that chooses its passes the way heavy_mi2 does (pcc_model2_fuzz_sweeps).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { double t1, lat; } rec_t;
typedef struct {
    double q, tu, t[2];
    uint32_t a[2], d[2];
} st2_t;

static uint32_t exp_bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return (uint32_t)((b >> 52) & 0x7FFu);
}
static double pow2(int e) {
    uint64_t b = (uint64_t)(e + 1023) << 52;
    double x;
    memcpy(&x, &b, 8);
    return x;
}
static double max0(double x) { return x > 0.0 ? x : 0.0; }

/* ns:66-84 */
static int link_send(double t, int rnd, double dl, double maxq, double ebw, double *q, double *tu, rec_t *rec) {
    const double qd = max0(*q - (t - *tu));
    rec->lat = dl + qd;
    rec->t1 = t + rec->lat;
    if (rnd) return 1;
    *q = qd;
    *tu = t;
    if (ebw + *q > maxq) return 1;
    *q += ebw;
    return 0;
}

/* up to `limit` packets of the merged stream by the plain recurrence; loss[k] = k-th packet of the interval is lost at random */
static uint32_t plain(st2_t *s, const double gap[2], double end, double dl, double maxq, double ebw, const uint8_t *loss,
                      uint32_t k0, uint32_t limit, rec_t *acc[2], rec_t *drp[2]) {
    uint32_t k = 0;
    while (k < limit) {
        const int sd = s->t[1] < s->t[0] ? 1 : 0;
        const double t = s->t[sd];
        if (!(t < end)) break;
        rec_t r;
        const int dropped = link_send(t, loss[k0 + k], dl, maxq, ebw, &s->q, &s->tu, &r);
        if (dropped) drp[sd][s->d[sd]++] = r;
        else acc[sd][s->a[sd]++] = r;
        s->t[sd] = t + gap[sd];
        k++;
    }
    return k;
}

static int g_lanes = 64, g_per_lane = 1;
int pcc_model2_set_shape(int lanes, int per_lane) {
    if (lanes < 1 || lanes > 1024 || per_lane < 1 || per_lane > 4) return -1;
    g_lanes = lanes;
    g_per_lane = per_lane;
    return 0;
}

#define MAXPOS 4096

/* one token pass; returns the packets it committed (0: preconditions not met / first packet flagged) */
static uint32_t token_pass(st2_t *st, const double gap[2], double end, double dl, double maxq, double ebw, const uint8_t *loss,
                           uint32_t k0, rec_t *acc[2], rec_t *drp[2], uint32_t *stopped_early) {
    const uint32_t kPass = (uint32_t)(g_lanes * g_per_lane);
    double G[2];
    int okb = 1;
    double tend_max = 0.0;
    for (int s = 0; s < 2; s++) {
        const double t0 = st->t[s], t1s = t0 + gap[s];
        G[s] = t1s - t0;
        const double t2s = t1s + gap[s], tend = t0 + (double)kPass * G[s];
        okb = okb && (t2s - t1s == G[s]) && (G[s] > 0.0) && (t0 >= ((double)kPass + 4.0) * gap[s]) && (exp_bits(t0) == exp_bits(tend));
        if (tend > tend_max) tend_max = tend;
    }
    const uint32_t e = exp_bits(st->q), eb = exp_bits(ebw);
    const double T0 = st->t[0] <= st->t[1] ? st->t[0] : st->t[1];
    const double x0 = st->q - (T0 - st->tu);
    okb = okb && (st->tu >= maxq) && (st->tu + st->tu >= tend_max) && (st->q > 0.0) && e > 64u && e < 1100u && (x0 > 0.0) && eb <= e &&
          exp_bits(st->tu) >= e && exp_bits(maxq) >= e;
    if (!okb) return 0;
    const double u = pow2((int)e - 1023 - 52), inv_u = pow2(-((int)e - 1023 - 52)), probe = pow2((int)e - 1023);
    const double R = (eb == e) ? ebw : (probe + ebw) - probe;
    const double err = ebw - R;
    const int tie = fabs(err) == 0.5 * u;
    if (!((tend_max - st->tu) * inv_u < 4.0e18 && R > 0.0)) return 0;
    const int64_t Q0i = (int64_t)(st->q * inv_u), Ri = (int64_t)(R * inv_u);
    int64_t Dsi[2], Gsi[2];
    for (int s = 0; s < 2; s++) {
        Dsi[s] = (int64_t)((st->t[s] - st->tu) * inv_u);
        Gsi[s] = (int64_t)(G[s] * inv_u);
    }
    const double room = ((maxq - R) - x0) / R;
    const int free_mode = room >= (double)kPass + 44.0;
    const int64_t Mi = free_mode ? 0 : (int64_t)(maxq * inv_u);
    if (tie && ((Q0i | Dsi[0] | Dsi[1] | Gsi[0] | Gsi[1]) & 1)) return 0;
    const int maxq_above = exp_bits(maxq) > e;

    /* the merged positions (the kernel finds them per lane by a merge-path search) */
    static double tk[MAXPOS];
    static int64_t Dp[MAXPOS];
    static int sd[MAXPOS], m[MAXPOS], ex[MAXPOS], N[MAXPOS + 1], a_[MAXPOS], accv[MAXPOS], flag[MAXPOS];
    uint32_t c[2] = {0, 0};
    for (uint32_t p = 0; p < kPass; p++) {
        const double A = st->t[0] + (double)c[0] * G[0], B = st->t[1] + (double)c[1] * G[1];
        const int is1 = !(A <= B);
        sd[p] = is1;
        tk[p] = is1 ? B : A;
        Dp[p] = Dsi[is1] + (int64_t)c[is1] * Gsi[is1];
        ex[p] = tk[p] < end;
        m[p] = ex[p] && !loss[k0 + p];
        c[is1]++;
    }
    /* accept decisions */
    if (free_mode) {
        for (uint32_t p = 0; p < kPass; p++) accv[p] = m[p];
    } else {
        for (uint32_t p = 0; p < kPass; p++) {
            const int64_t num = (Mi - Q0i) + Dp[p];
            int n = (int)((double)num * (1.0 / (double)Ri));
            int64_t rem = num - (int64_t)n * Ri;
            if (rem < 0) { n--; rem += Ri; }
            if (rem >= Ri) { n++; }
            N[p] = n;
        }
        N[kPass] = N[kPass - 1];   /* (the last lane's last position: no arrival behind it) */
        /* the kernel: per-lane composites + prefix scan; here the same Lindley recursion, position by position */
        int b = N[0];
        for (uint32_t p = 0; p < kPass; p++) {
            a_[p] = N[p + 1] - N[p];
            accv[p] = m[p] && b > 0;
            b = (b - m[p] > 0 ? b - m[p] : 0) + a_[p];
        }
    }
    int j = 0;
    uint32_t p_stop = kPass;
    static double xq[MAXPOS];
    for (uint32_t p = 0; p < kPass; p++) {
        const int64_t xi = Q0i + (int64_t)j * Ri - Dp[p];
        xq[p] = (double)xi * u;
        const double sx = xq[p] + R;
        const uint32_t es = exp_bits(sx);
        flag[p] = m[p] && (!(xq[p] > 0.0) || es < e || (es > e && maxq_above));
        if ((!ex[p] || flag[p]) && p < p_stop) p_stop = p;
        j += accv[p];
    }
    *stopped_early = p_stop < kPass && ex[p_stop < kPass ? p_stop : 0];
    if (!p_stop) return 0;
    uint32_t n[2] = {0, 0};
    for (uint32_t p = 0; p < p_stop; p++) {
        rec_t r;
        r.lat = dl + max0(xq[p]);
        r.t1 = tk[p] + r.lat;
        if (accv[p]) acc[sd[p]][st->a[sd[p]]++] = r;
        else drp[sd[p]][st->d[sd[p]]++] = r;
        if (m[p]) { st->q = accv[p] ? xq[p] + R : xq[p]; st->tu = tk[p]; }
        n[sd[p]]++;
    }
    st->t[0] = st->t[0] + (double)n[0] * G[0];
    st->t[1] = st->t[1] + (double)n[1] * G[1];
    return p_stop;
}

static uint64_t fz = 88172645463325252ull;
static uint64_t fz_next(void) { fz ^= fz << 13; fz ^= fz >> 7; fz ^= fz << 17; return fz; }
static double fz_unit(void) { return (double)(fz_next() >> 11) * (1.0 / 9007199254740992.0); }

#define MAXPK 40000

/* n_cases random link states and intervals; returns the number of mismatching cases.  stats: [0] token passes that
 * committed, [1] packets they committed, [2] packets sent by the plain recurrence, [3] passes stopped early by a flag */
long pcc_model2_fuzz(long n_cases, uint64_t seed, uint64_t *stats) {
    fz = seed ? seed : 1;
    long bad = 0;
    static rec_t ra[2][2][MAXPK], rd[2][2][MAXPK];
    static uint8_t loss[MAXPK + 8192];
    for (int k = 0; k < 4; k++) stats[k] = 0;
    for (long cs = 0; cs < n_cases; cs++) {
        const double bw = 100.0 + 400.0 * fz_unit();
        const double ebw = 1.0 / bw;
        double queue = 1.0 + floor(exp(8.0 * fz_unit()));
        if (fz_unit() < 0.35) {   /* queue limits around powers of two (in seconds) */
            const double B = pow2((int)(fz_next() % 8) - 3);
            queue = floor(B * bw + 6.0 * fz_unit() - 3.0);
            if (queue < 2.0) queue = 2.0;
        }
        const double maxq = queue / bw;
        const double dl = 0.05 + 0.45 * fz_unit();
        const double lr = fz_unit() < 0.25 ? 0.0 : 0.05 * fz_unit();
        const double load = fz_unit() < 0.7 ? 1.02 + 0.8 * fz_unit() : 0.4 + 1.2 * fz_unit();
        const double share = 0.2 + 0.6 * fz_unit();
        double rate[2] = {bw * load * share, bw * load * (1.0 - share)};
        for (int s = 0; s < 2; s++) { if (rate[s] < 40.0) rate[s] = 40.0; if (rate[s] > 1000.0) rate[s] = 1000.0; }
        const double gap[2] = {1.0 / rate[0], 1.0 / rate[1]};
        /* a clock somewhere in an episode (young episodes included), the queue anywhere up to full */
        const double now = fz_unit() < 0.2 ? 0.05 + 3.0 * fz_unit() : 3.0 + 400.0 * fz_unit();
        st2_t s0;
        s0.tu = now - ebw * fz_unit();
        s0.q = fz_unit() < 0.2 ? maxq * fz_unit() : (fz_unit() < 0.5 ? maxq - ebw * 3.0 * fz_unit() : maxq * (0.5 + 0.5 * fz_unit()));
        if (s0.q < 0.0) s0.q = 0.0;
        s0.t[0] = now + gap[0] * fz_unit();
        s0.t[1] = now + gap[1] * fz_unit();
        if (fz_unit() < 0.1) s0.t[1] = s0.t[0];   /* equal times: sender 0 first */
        s0.a[0] = s0.a[1] = s0.d[0] = s0.d[1] = 0;
        const double end = now + (0.05 + 2.0 * fz_unit());
        for (int k = 0; k < MAXPK + 8192; k++) loss[k] = fz_unit() < lr;
        if ((rate[0] + rate[1]) * (end - now) > (double)MAXPK - 100.0) continue;
        /* reference */
        st2_t r = s0;
        rec_t *racc[2] = {ra[0][0], ra[0][1]}, *rdrp[2] = {rd[0][0], rd[0][1]};
        uint32_t kr = 0;
        for (;;) {
            const uint32_t n = plain(&r, gap, end, dl, maxq, ebw, loss, kr, 1u << 30, racc, rdrp);
            kr += n;
            break;
        }
        /* model */
        st2_t md = s0;
        rec_t *macc[2] = {ra[1][0], ra[1][1]}, *mdrp[2] = {rd[1][0], rd[1][1]};
        uint32_t km = 0, chain_left = 0, guard = 0;
        while ((md.t[0] < md.t[1] ? md.t[0] : md.t[1]) < end) {
            if (++guard > 100000u) { km = 0xFFFFFFFFu; break; }
            uint32_t n = 0, early = 0;
            if (chain_left) chain_left--;
            else {
                n = token_pass(&md, gap, end, dl, maxq, ebw, loss, km, macc, mdrp, &early);
                if (early && n < (uint32_t)(g_per_lane > 1 ? 32 : 16)) chain_left = 2;
                if (n) { stats[0]++; stats[1] += n; stats[3] += early; }
            }
            if (!n) {
                n = plain(&md, gap, end, dl, maxq, ebw, loss, km, 64, macc, mdrp);
                stats[2] += n;
            }
            km += n;
        }
        int same = km == kr && md.q == r.q && md.tu == r.tu && md.t[0] == r.t[0] && md.t[1] == r.t[1];
        for (int s = 0; s < 2 && same; s++) {
            same = md.a[s] == r.a[s] && md.d[s] == r.d[s] && !memcmp(ra[0][s], ra[1][s], sizeof(rec_t) * r.a[s]) &&
                   !memcmp(rd[0][s], rd[1][s], sizeof(rec_t) * r.d[s]);
        }
        if (!same) bad++;
    }
    return bad;
}


/* ======================================================================================================================
 * The sweep formulations of heavy_mi2.  A wavefront of kLanes lanes; every lane holds the link state BEHIND its positions;
 * one sweep = every lane takes the state of the lane below it (lane 0: the state the pass starts from) and redoes its own
 * positions with the reference's expressions (ns:66-82); a sweep that moves no lane's state has reached the fixed point, which
 * is the serial recurrence.  Neither formulation asks for tu >= maxq or tu + tu >= tend_max: only the send times must be
 * exact (two equal increments, a clock old enough, no binade crossing inside the pass -- positions from the top of the
 * binade of either sender's send time on are not part of the pass).
 * ====================================================================================================================== */
#define kLanes 64

typedef struct {   /* what one pass did, for the statistics */
    uint32_t committed, sweeps;
} sweep_out_t;

static double top_of_binade(double t0) { return pow2((int)exp_bits(t0) - 1022); }

/* the 256-position sweep pass (pcc_wave_pass.h, "sweep pass"): lane l owns the positions 4 l .. 4 l + 3, the first `skip` of
 * lane 0 were sent before (a Philox block holds four packets of the interval); k0 = packets of the interval sent so far.
 * Returns 0 when the send-time preconditions do not hold. */
static int sweep256_pass(st2_t *st, const double gap[2], double end, double dl, double maxq, double ebw, const uint8_t *loss,
                         uint32_t k0, rec_t *acc[2], rec_t *drp[2], sweep_out_t *out) {
    const uint32_t kPass = 4u * kLanes;
    double G[2], lim = end;
    int okt = 1;
    for (int s = 0; s < 2; s++) {
        const double t0 = st->t[s], t1s = t0 + gap[s];
        G[s] = t1s - t0;
        const double t2s = t1s + gap[s], ttop = top_of_binade(t0);
        if (ttop < lim) lim = ttop;
        okt = okt && (t2s - t1s == G[s]) && (G[s] > 0.0) && (t0 >= ((double)kPass + 4.0) * gap[s]) && (exp_bits(t0) == exp_bits(t2s));
    }
    out->committed = out->sweeps = 0;
    if (!okt) return 0;
    const uint32_t skip = k0 & 3u;
    /* per lane: send time, sender, "holds a packet of this interval", "... that reaches the queue" of its four positions */
    static double tk[kLanes][4];
    static int sd[kLanes][4], ex[kLanes][4], m[kLanes][4];
    for (uint32_t l = 0; l < kLanes; l++) {
        const int kbase = 4 * (int)l - (int)skip;
        const uint32_t kf = kbase < 0 ? 0u : (uint32_t)kbase;
        /* merge path: smallest c with B[kf - c - 1] < A[c] (sender 0 first on equal times) */
        uint32_t lo = 0, hi = kf;
        while (lo < hi) {
            const uint32_t c = (lo + hi) >> 1;
            const double Ac = st->t[0] + (double)c * G[0], Bp = st->t[1] + (double)(kf - c - 1u) * G[1];
            if (Bp < Ac) hi = c;
            else lo = c + 1u;
        }
        uint32_t c0 = lo, c1 = kf - lo;
        for (int i = 0; i < 4; i++) {
            const double A = st->t[0] + (double)c0 * G[0], B = st->t[1] + (double)c1 * G[1];
            const int is1 = !(A <= B), there = kbase + i >= 0;
            tk[l][i] = is1 ? B : A;
            sd[l][i] = is1;
            ex[l][i] = there && tk[l][i] < lim;
            m[l][i] = ex[l][i] && !loss[k0 + (uint32_t)(there ? kbase + i : 0)];
            if (there) { c0 += is1 ? 0u : 1u; c1 += is1 ? 1u : 0u; }
        }
    }
    /* the sweeps: sweep 0 starts every lane from "the lane below left the queue drained" */
    static double sw_q[kLanes], sw_t[kLanes], xq[kLanes][4];
    static int a4[kLanes][4];
    for (uint32_t l = 0; l < kLanes; l++) { sw_q[l] = 0.0; sw_t[l] = 0.0; }
    for (uint32_t sweep = 0; sweep <= kLanes; sweep++) {
        double nq[kLanes], nt[kLanes];
        int any = 0;
        for (uint32_t l = 0; l < kLanes; l++) {
            double q = 0.0, t = st->tu;
            if (sweep) { q = l ? sw_q[l - 1] : st->q; t = l ? sw_t[l - 1] : st->tu; }
            for (int i = 0; i < 4; i++) {
                const double qc = max0(q - (tk[l][i] - t));
                const int a = m[l][i] && !(ebw + qc > maxq);
                xq[l][i] = qc;
                a4[l][i] = a;
                q = m[l][i] ? (a ? ebw + qc : qc) : q;
                t = m[l][i] ? tk[l][i] : t;
            }
            const int moved = memcmp(&q, &sw_q[l], 8) != 0 || memcmp(&t, &sw_t[l], 8) != 0 || sweep == 0u;
            any |= moved;
            nq[l] = q;
            nt[l] = t;
        }
        memcpy(sw_q, nq, sizeof nq);
        memcpy(sw_t, nt, sizeof nt);
        out->sweeps++;
        if (sweep && !any) break;
    }
    /* the pass stops at the first position past the interval's end (or the top of the binade) */
    uint32_t p_stop = kPass;
    for (uint32_t p = skip; p < kPass; p++)
        if (!ex[p >> 2][p & 3u]) { p_stop = p; break; }
    const uint32_t ncommit = p_stop - skip;
    if (!ncommit) return 1;
    uint32_t n[2] = {0, 0};
    for (uint32_t p = skip; p < p_stop; p++) {
        const uint32_t l = p >> 2, i = p & 3u;
        rec_t r;
        r.lat = dl + max0(xq[l][i]);
        r.t1 = tk[l][i] + r.lat;
        if (a4[l][i]) acc[sd[l][i]][st->a[sd[l][i]]++] = r;
        else drp[sd[l][i]][st->d[sd[l][i]]++] = r;
        if (m[l][i]) { st->q = a4[l][i] ? xq[l][i] + ebw : xq[l][i]; st->tu = tk[l][i]; }
        n[sd[l][i]]++;
    }
    if (n[0]) st->t[0] = (st->t[0] + (double)(n[0] - 1u) * G[0]) + gap[0];
    if (n[1]) st->t[1] = (st->t[1] + (double)(n[1] - 1u) * G[1]) + gap[1];
    out->committed = ncommit;
    return 1;
}

/* the 64-lane pass settled side by side (pcc_wave_pass.h, "phase 1, side by side"): lane l owns merged position l; the first
 * guess is "every packet found the queue drained"; four sweeps between two looks at whether anything still moves.
 * Returns 0 when the send-time preconditions do not hold (the kernel then runs the plain recurrence). */
static int sweep64_pass(st2_t *st, const double gap[2], double end, double dl, double maxq, double ebw, const uint8_t *loss,
                        uint32_t k0, rec_t *acc[2], rec_t *drp[2], sweep_out_t *out) {
    double G[2], lim = end;
    int ok = 1;
    for (int s = 0; s < 2; s++) {
        const double t0 = st->t[s], t1s = t0 + gap[s];
        G[s] = t1s - t0;
        const double t2s = t1s + gap[s], ttop = top_of_binade(t0);
        if (ttop < lim) lim = ttop;
        ok = ok && (t2s - t1s == G[s]) && (t0 >= 128.0 * gap[s]) && (exp_bits(t0) == exp_bits(t2s)) && (G[s] > 0.0);
    }
    out->committed = out->sweeps = 0;
    if (!ok) return 0;
    double tk[kLanes], oq[kLanes], ot[kLanes], qc[kLanes];
    int sdr[kLanes], valid[kLanes], mine[kLanes], full[kLanes];
    uint32_t nv = 0;
    for (uint32_t l = 0; l < kLanes; l++) {
        uint32_t lo = 0, hi = l;
        while (lo < hi) {
            const uint32_t c = (lo + hi) >> 1;
            const double Ac = st->t[0] + (double)c * G[0], Bp = st->t[1] + (double)(l - c - 1) * G[1];
            if (Bp < Ac) hi = c;
            else lo = c + 1;
        }
        const uint32_t c0 = lo, c1 = l - lo;
        const double A = st->t[0] + (double)c0 * G[0], B = st->t[1] + (double)c1 * G[1];
        sdr[l] = (A <= B) ? 0 : 1;
        tk[l] = sdr[l] ? B : A;
        valid[l] = tk[l] < lim;
        nv += valid[l] ? 1u : 0u;
        mine[l] = valid[l] && !loss[k0 + l];
        full[l] = 0;
        qc[l] = 0.0;
    }
    /* first guess: the state behind a lane = (1/bw, the send time of the last packet up to it that reaches the queue) */
    int gl = -1;
    for (uint32_t l = 0; l < kLanes; l++) {
        if (mine[l]) gl = (int)l;
        oq[l] = gl >= 0 ? ebw : st->q;
        ot[l] = gl >= 0 ? tk[gl] : st->tu;
    }
    for (uint32_t sweep = 0; sweep < nv; sweep += 4u) {
        int any = 0;
        for (int r = 0; r < 4; r++) {
            double nq[kLanes], nt[kLanes];
            for (uint32_t l = 0; l < kLanes; l++) {
                const double iq = l ? oq[l - 1] : st->q, it = l ? ot[l - 1] : st->tu;
                qc[l] = max0(iq - (tk[l] - it));
                full[l] = ebw + qc[l] > maxq;
                nq[l] = mine[l] ? (full[l] ? qc[l] : ebw + qc[l]) : iq;
                nt[l] = mine[l] ? tk[l] : it;
                if (r == 3) any |= valid[l] && (memcmp(&nq[l], &oq[l], 8) != 0 || memcmp(&nt[l], &ot[l], 8) != 0);
            }
            memcpy(oq, nq, sizeof nq);
            memcpy(ot, nt, sizeof nt);
        }
        out->sweeps += 4;
        if (!any) break;
    }
    uint32_t n[2] = {0, 0};
    for (uint32_t l = 0; l < nv; l++) {   /* (merged times increase: the valid lanes are a prefix) */
        const int dropped = !(mine[l] && !full[l]);
        rec_t r;
        r.lat = dl + qc[l];
        r.t1 = tk[l] + r.lat;
        if (dropped) drp[sdr[l]][st->d[sdr[l]]++] = r;
        else acc[sdr[l]][st->a[sdr[l]]++] = r;
        n[sdr[l]]++;
    }
    for (int l = (int)nv - 1; l >= 0; l--)
        if (mine[l]) { st->q = full[l] ? qc[l] : ebw + qc[l]; st->tu = tk[l]; break; }
    if (n[0]) st->t[0] = (st->t[0] + (double)(n[0] - 1u) * G[0]) + gap[0];
    if (n[1]) st->t[1] = (st->t[1] + (double)(n[1] - 1u) * G[1]) + gap[1];
    out->committed = nv;
    return 1;
}

/* one fuzzed link, pair of senders and interval: the generators of pcc_model2_fuzz_sweeps (see there), kind 0 .. 3 */
typedef struct { int kind; double ebw, maxq, dl, lr, now, end, rate[2], gap[2]; st2_t s0; } gen2_t;
static void gen2_sweeps(gen2_t *g) {
    const double bw = 100.0 + 400.0 * fz_unit();
    const double ebw = 1.0 / bw;
    const int kind = (int)(fz_next() % 4u);   /* 0, 1: the generators of pcc_model2_fuzz; 2: (a); 3: (b) */
    double queue = 1.0 + floor(exp(8.0 * fz_unit()));
    if (fz_unit() < 0.35) {   /* queue limits around powers of two (in seconds) */
        const double B = pow2((int)(fz_next() % 8) - 3);
        queue = floor(B * bw + 6.0 * fz_unit() - 3.0);
        if (queue < 2.0) queue = 2.0;
    }
    if (kind == 3) queue = 2000.0 + floor(1000.0 * fz_unit());
    const double maxq = queue / bw;
    const double dl = 0.05 + 0.45 * fz_unit();
    double lr = fz_unit() < 0.25 ? 0.0 : 0.05 * fz_unit();
    double load = fz_unit() < 0.7 ? 1.02 + 0.8 * fz_unit() : 0.4 + 1.2 * fz_unit();
    double share = 0.2 + 0.6 * fz_unit();
    if (kind == 2) { load = 0.3 + 0.65 * fz_unit(); if (fz_unit() < 0.5) share = 0.5; }
    if (kind == 3) { load = 1.2 + 0.4 * fz_unit(); lr = 0.0; }
    double rate[2] = {bw * load * share, bw * load * (1.0 - share)};
    for (int s = 0; s < 2; s++) { if (rate[s] < 40.0) rate[s] = 40.0; if (rate[s] > 1000.0) rate[s] = 1000.0; }
    const double gap[2] = {1.0 / rate[0], 1.0 / rate[1]};
    double now = fz_unit() < 0.2 ? 0.05 + 3.0 * fz_unit() : 3.0 + 400.0 * fz_unit();
    if (kind == 3 && fz_unit() < 0.5) {   /* old enough for 64 positions, too young for 256 */
        const double gmax = gap[0] > gap[1] ? gap[0] : gap[1];
        now = gmax * (130.0 + 120.0 * fz_unit());
    }
    st2_t s0;
    s0.tu = now - ebw * fz_unit();
    s0.q = fz_unit() < 0.2 ? maxq * fz_unit() : (fz_unit() < 0.5 ? maxq - ebw * 3.0 * fz_unit() : maxq * (0.5 + 0.5 * fz_unit()));
    if (kind == 2) s0.q = fz_unit() < 0.5 ? 0.0 : ebw * 2.0 * fz_unit();
    if (kind == 3) s0.q = maxq * (0.4 + 0.2 * fz_unit());
    if (s0.q < 0.0) s0.q = 0.0;
    s0.t[0] = now + gap[0] * fz_unit();
    s0.t[1] = now + gap[1] * fz_unit();
    if (fz_unit() < 0.1 || (kind == 2 && fz_unit() < 0.5)) s0.t[1] = s0.t[0];   /* equal times: sender 0 first */
    s0.a[0] = s0.a[1] = s0.d[0] = s0.d[1] = 0;
    const double end = now + (0.05 + 2.0 * fz_unit());
    g->kind = kind; g->ebw = ebw; g->maxq = maxq; g->dl = dl; g->lr = lr; g->now = now; g->end = end;
    g->rate[0] = rate[0]; g->rate[1] = rate[1]; g->gap[0] = gap[0]; g->gap[1] = gap[1]; g->s0 = s0;
}

/* n_cases random link states and intervals through heavy_mi2's choice of passes -- the token pass where its preconditions
 * hold (use_token != 0; after a short one the next three passes go by sweeps), else the 256-position sweep pass, else the
 * 64-lane sweep pass, else the plain recurrence -- against the plain recurrence alone; returns the number of mismatching cases.
 * Generators: those of pcc_model2_fuzz (pairs that overdrive the link, queue limits around powers of two, young and old
 * clocks, equal send times) and, one case in four each, (a) links that keep running empty -- the pair sends at 30..95 % of
 * the link's rate, in step, so every few packets find the queue drained: what stops a token pass -- and (b) one busy period
 * over the whole pass with nothing that forgets the state it started from: a deep queue half full, no random loss, the pair
 * at 1.2..1.6 times the link's rate, the clock young enough for the 64-lane pass in half of them -- no early fixed point.
 * stats: [0] token passes, [1] their packets, [2] 256-position sweep passes, [3] their packets, [4] their sweeps, [5] the
 * most sweeps one of them took, [6] 64-lane sweep passes, [7] their packets, [8] their sweeps, [9] the most sweeps one of
 * them took, [10] plain passes, [11] their packets, [12] cases of generator (a), [13] of generator (b). */
long pcc_model2_fuzz_sweeps(long n_cases, uint64_t seed, int use_token, uint64_t *stats) {
    fz = seed ? seed : 1;
    long bad = 0;
    static rec_t ra[2][2][MAXPK], rd[2][2][MAXPK];
    static uint8_t loss[MAXPK + 8192];
    const int lanes0 = g_lanes, per0 = g_per_lane;
    g_lanes = 64; g_per_lane = 4;   /* the kernel's token pass: 256 positions */
    for (int k = 0; k < 14; k++) stats[k] = 0;
    for (long cs = 0; cs < n_cases; cs++) {
        gen2_t g2;
        gen2_sweeps(&g2);
        const int kind = g2.kind;
        const double ebw = g2.ebw, maxq = g2.maxq, dl = g2.dl, lr = g2.lr, now = g2.now, end = g2.end;
        const double rate[2] = {g2.rate[0], g2.rate[1]}, gap[2] = {g2.gap[0], g2.gap[1]};
        const st2_t s0 = g2.s0;
        for (int k = 0; k < MAXPK + 8192; k++) loss[k] = fz_unit() < lr;
        if ((rate[0] + rate[1]) * (end - now) > (double)MAXPK - 100.0) continue;
        stats[12] += kind == 2;
        stats[13] += kind == 3;
        /* reference */
        st2_t r = s0;
        rec_t *racc[2] = {ra[0][0], ra[0][1]}, *rdrp[2] = {rd[0][0], rd[0][1]};
        const uint32_t kr = plain(&r, gap, end, dl, maxq, ebw, loss, 0, 1u << 30, racc, rdrp);
        /* model: heavy_mi2's loop */
        st2_t md = s0;
        rec_t *macc[2] = {ra[1][0], ra[1][1]}, *mdrp[2] = {rd[1][0], rd[1][1]};
        uint32_t km = 0, chain_left = 0, guard = 0;
        while ((md.t[0] < md.t[1] ? md.t[0] : md.t[1]) < end) {
            if (++guard > 100000u) { km = 0xFFFFFFFFu; break; }
            uint32_t n = 0, early = 0;
            const int held = chain_left != 0u;
            if (chain_left) chain_left--;
            /* (the model's token pass has no positions sent before it: it is tried on whole Philox blocks only) */
            if (use_token && !held && (km & 3u) == 0u) {
                n = token_pass(&md, gap, end, dl, maxq, ebw, loss, km, macc, mdrp, &early);
                if (n) { stats[0]++; stats[1] += n; }
                if (n && early && n < 32u) chain_left = 3;
            }
            sweep_out_t so;
            if (!n && sweep256_pass(&md, gap, end, dl, maxq, ebw, loss, km, macc, mdrp, &so)) {
                n = so.committed;
                if (n) { stats[2]++; stats[3] += n; }
                stats[4] += so.sweeps;
                if (so.sweeps > stats[5]) stats[5] = so.sweeps;
            }
            if (!n && sweep64_pass(&md, gap, end, dl, maxq, ebw, loss, km, macc, mdrp, &so)) {
                n = so.committed;
                stats[6]++; stats[7] += n; stats[8] += so.sweeps;
                if (so.sweeps > stats[9]) stats[9] = so.sweeps;
                if (!n) { km = 0xFFFFFFFFu; break; }   /* (a pass that commits nothing would never end) */
            }
            if (!n) {
                n = plain(&md, gap, end, dl, maxq, ebw, loss, km, 64, macc, mdrp);
                stats[10]++; stats[11] += n;
            }
            km += n;
        }
        int same = km == kr && md.q == r.q && md.tu == r.tu && md.t[0] == r.t[0] && md.t[1] == r.t[1];
        for (int s = 0; s < 2 && same; s++) {
            same = md.a[s] == r.a[s] && md.d[s] == r.d[s] && !memcmp(ra[0][s], ra[1][s], sizeof(rec_t) * r.a[s]) &&
                   !memcmp(rd[0][s], rd[1][s], sizeof(rec_t) * r.d[s]);
        }
        if (!same) bad++;
    }
    g_lanes = lanes0; g_per_lane = per0;
    return bad;
}

/* ======================================================================================================================
 * Entries for the case tables of tests/models/send_pass_cases.py (the device tests of heavy_mi2, tests/test_send_pass_device.py):
 * cases go in and out as arrays, nothing here asserts.
 * ====================================================================================================================== */
typedef struct { double q, tu, t[2], dl, lr, maxq, ebw, gap[2], end; uint32_t sent[2]; } mcase2_t;   /* 96 bytes */

/* (a) n cases of the generators of pcc_model2_fuzz_sweeps: kind 0 .. 3 as drawn (kind_only < 0) or only the cases of one kind
 * (2: the link keeps running empty, 3: one busy period over the pass); both senders' intervals cut to max_packets packets each.
 * kinds_out[c]: the kind of case c. */
long pcc_cases2_fuzz(long n, uint64_t seed, int kind_only, double max_packets, mcase2_t *out, int32_t *kinds_out) {
    fz = seed ? seed : 1;
    long c = 0, guard = 0;
    while (c < n && guard++ < 100 * n + 1000) {
        gen2_t g;
        gen2_sweeps(&g);
        if (kind_only >= 0 && g.kind != kind_only) continue;
        double end = g.end;
        for (int s = 0; s < 2; s++)
            if ((end - g.s0.t[s]) / g.gap[s] > max_packets) end = g.s0.t[s] + max_packets * g.gap[s];
        mcase2_t *o = &out[c];
        o->q = g.s0.q; o->tu = g.s0.tu; o->dl = g.dl; o->lr = g.lr; o->maxq = g.maxq; o->ebw = g.ebw; o->end = end;
        for (int s = 0; s < 2; s++) { o->t[s] = g.s0.t[s]; o->gap[s] = g.gap[s]; o->sent[s] = 0; }
        o->sent[0] = (uint32_t)(fz_next() & 3u);   /* Philox block alignment of a take-over */
        if (kinds_out) kinds_out[c] = g.kind;
        c++;
    }
    return c;
}

static long case2_packets(const mcase2_t *c, long room) {
    long k = 0;
    for (int s = 0; s < 2; s++) {
        double t = c->t[s];
        if (!(c->gap[s] > 0.0) || !(t + c->gap[s] > t)) return -1;
        while (t < c->end) {
            if (++k > room) return -1;
            t += c->gap[s];
        }
    }
    return k;
}

/* (b) the plain merged recurrence (plain) on n cases.  Case c owns the elements [off[c], off[c + 1]) of loss (loss[off[c] + k]:
 * the k-th packet of the merged stream is lost at random) and of the four record arrays (sender x accepted / dropped, each in
 * send order).  out[c]: the final state, a / d counted from 0.  Returns 0, or -(c + 1) for the first case that does not fit. */
long pcc_cases2_plain(long n, const mcase2_t *cs, const uint8_t *loss, const int64_t *off, st2_t *out, rec_t *acc0, rec_t *drp0,
                      rec_t *acc1, rec_t *drp1) {
    for (long c = 0; c < n; c++) {
        if (case2_packets(&cs[c], (long)(off[c + 1] - off[c])) < 0) return -(c + 1);
        st2_t s;
        memset(&s, 0, sizeof s);
        s.q = cs[c].q; s.tu = cs[c].tu; s.t[0] = cs[c].t[0]; s.t[1] = cs[c].t[1];
        rec_t *acc[2] = {acc0 + off[c], acc1 + off[c]}, *drp[2] = {drp0 + off[c], drp1 + off[c]};
        plain(&s, cs[c].gap, cs[c].end, cs[c].dl, cs[c].maxq, cs[c].ebw, loss + off[c], 0, 1u << 30, acc, drp);
        out[c] = s;
    }
    return 0;
}

#define MIRROR2_COLS 8
/* (c) the mirror: heavy_mi2's choice of passes as pcc_model2_fuzz_sweeps drives it (the token pass on whole Philox blocks, then
 * the 256-position sweep pass, the 64-lane sweep pass, the plain recurrence).  counts[c][MIRROR2_COLS]: passes / packets of the
 * token pass (0, 1), the 256-position sweeps (2, 3), the 64-lane sweeps (4, 5), the plain recurrence (6, 7). */
long pcc_cases2_mirror(long n, const mcase2_t *cs, const uint8_t *loss, const int64_t *off, st2_t *out, rec_t *acc0, rec_t *drp0,
                       rec_t *acc1, rec_t *drp1, uint64_t *counts) {
    const int lanes0 = g_lanes, per0 = g_per_lane;
    g_lanes = 64; g_per_lane = 4;
    long rc = 0;
    for (long c = 0; c < n; c++) {
        if (case2_packets(&cs[c], (long)(off[c + 1] - off[c])) < 0) { rc = -(c + 1); break; }
        const mcase2_t *C = &cs[c];
        st2_t md;
        memset(&md, 0, sizeof md);
        md.q = C->q; md.tu = C->tu; md.t[0] = C->t[0]; md.t[1] = C->t[1];
        rec_t *macc[2] = {acc0 + off[c], acc1 + off[c]}, *mdrp[2] = {drp0 + off[c], drp1 + off[c]};
        const uint32_t base = C->sent[0] + C->sent[1];            /* packets of the interval sent before the case begins */
        const uint8_t *ls = loss + off[c] - base;                 /* ls[packet index of the interval] */
        uint64_t *k = counts + c * MIRROR2_COLS;
        for (int i = 0; i < MIRROR2_COLS; i++) k[i] = 0;
        uint32_t km = base, chain_left = 0, guard = 0;
        while ((md.t[0] < md.t[1] ? md.t[0] : md.t[1]) < C->end) {
            if (++guard > 100000u) { rc = -(c + 1); break; }
            uint32_t m = 0, early = 0;
            const int held = chain_left != 0u;
            if (chain_left) chain_left--;
            if (!held && (km & 3u) == 0u) {
                m = token_pass(&md, C->gap, C->end, C->dl, C->maxq, C->ebw, ls, km, macc, mdrp, &early);
                if (m) { k[0]++; k[1] += m; }
                if (m && early && m < 32u) chain_left = 3;
            }
            sweep_out_t so;
            if (!m && sweep256_pass(&md, C->gap, C->end, C->dl, C->maxq, C->ebw, ls, km, macc, mdrp, &so)) {
                m = so.committed;
                if (m) { k[2]++; k[3] += m; }
            }
            if (!m && sweep64_pass(&md, C->gap, C->end, C->dl, C->maxq, C->ebw, ls, km, macc, mdrp, &so)) {
                m = so.committed;
                k[4]++; k[5] += m;
                if (!m) { rc = -(c + 1); break; }
            }
            if (!m) {
                m = plain(&md, C->gap, C->end, C->dl, C->maxq, C->ebw, ls, km, 64, macc, mdrp);
                k[6]++; k[7] += m;
            }
            km += m;
        }
        if (rc) break;
        out[c] = md;
    }
    g_lanes = lanes0; g_per_lane = per0;
    return rc;
}
