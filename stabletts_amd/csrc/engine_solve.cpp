// The ODE solve behind st_cfm_solve (include/stabletts_hip.h): torchdiffeq's fixed-grid solvers over one or more solve parts on
// as many streams, eager or replayed from a HIP graph, and the adaptive Runge-Kutta pairs and implicit Adams with their host-side
// controllers.  Reference path: models/flow_matching.py:25-67 (CFMDecoder.forward, cfg_wrapper), torchdiffeq's solvers.
#include "engine_dit.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

using namespace st;

namespace sthost {
namespace {

constexpr int kPartPhaseUs = 100;      // start offset between the launch sequences of a multi-part solve (solve_body)
// Default of the two-part solve (see solve_part_count): -1 = automatic (large fixed-grid batches), 1 = never.
constexpr int kDefaultSplit = -1;

// torch.linspace(0, 1, n + 1) in fp32 (CPU kernel: symmetric fill from both ends)
std::vector<float> linspace01(int n) {
    const int steps = n + 1;
    std::vector<float> t(steps);
    const float step = (1.0f - 0.0f) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i) t[i] = i < half ? 0.0f + step * (float)i : 1.0f - step * (float)(steps - i - 1);
    return t;
}

// ---------------------------------------------------------------------------------------------
// torchdiffeq's explicit ADAPTIVE Runge-Kutta solvers: `dopri5` -- the reference's default
// (models/flow_matching.py:54 with solver=None; rtol = atol = 1e-5 hard-coded there) -- and the other embedded
// pairs the reference's web UI offers (webui.py:110: bosh3, fehlberg2, adaptive_heun).  Restated from the
// published algorithm (rk_common.py / dopri5.py / bosh3.py / fehlberg2.py / adaptive_heun.py / misc.py of
// torchdiffeq 0.2.x): RMS error norm over the whole state tensor, controller safety 0.9 / ifactor 10 / dfactor
// 0.2 with exponent 1/order, initial step from _select_initial_step(order - 1), steps NOT clipped to t = 1 and the
// result taken from the 4th-order dense output (_interp_fit with f0 = k[0], f1 = k[-1]); like torchdiffeq the
// derivative carried into the next step is k[-1] whether or not the tableau is FSAL.
// The state, stage derivatives and norms live on the device; time and the controller run on the host
// (float64), with one 8-byte read-back per step (torchdiffeq synchronises the same way).
struct RkTableau {
    const char* name; int n; int order;       // n stages after k0 (k has n + 1 entries)
    double alpha[6]; double beta[6][6]; double csol[7]; double cerr[7]; double cmid[7];
};
static const RkTableau kDopri5 = {
    "dopri5", 6, 5,
    {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0},
    {{1.0 / 5},
     {3.0 / 40, 9.0 / 40},
     {44.0 / 45, -56.0 / 15, 32.0 / 9},
     {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
     {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
     {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}},
    {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0.0},
    {35.0 / 384 - 1951.0 / 21600, 0.0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
     -2187.0 / 6784 + 12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60},
    {6025192743.0 / 30085553152.0 / 2, 0.0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
     187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2}};
static const RkTableau kBosh3 = {
    "bosh3", 3, 3,
    {1.0 / 2, 3.0 / 4, 1.0},
    {{1.0 / 2}, {0.0, 3.0 / 4}, {2.0 / 9, 1.0 / 3, 4.0 / 9}},
    {2.0 / 9, 1.0 / 3, 4.0 / 9, 0.0},
    {2.0 / 9 - 7.0 / 24, 1.0 / 3 - 1.0 / 4, 4.0 / 9 - 1.0 / 3, -1.0 / 8},
    {0.0, 0.5, 0.0, 0.0}};
static const RkTableau kFehlberg2 = {
    "fehlberg2", 2, 2,
    {1.0 / 2, 1.0},
    {{1.0 / 2}, {1.0 / 256, 255.0 / 256}},
    {1.0 / 512, 255.0 / 256, 1.0 / 512},
    {-1.0 / 512, 0.0, 1.0 / 512},
    {0.0, 0.5, 0.0}};
static const RkTableau kAdaptiveHeun = {
    "adaptive_heun", 1, 2,
    {1.0}, {{1.0}}, {0.5, 0.5}, {0.5, -0.5}, {0.5, 0.0}};

// f(t, state in p.x16) -> kout for the host-controlled solvers (the time tables are rebuilt per evaluation)
int eval_rhs(st_engine* e, const Plan& p, const float* mask, int use_cfg, float cfg_strength, float t, float* kout, hipStream_t s) {
    DitState* dit = dit_of(e);
    HIPCHK(e, launch_set_scalar(p.tvals, t, s));
    int r = run_time_tables(e, p, s); if (r) return r;
    r = run_estimator(e, p, mask, 0, s); if (r) return r;
    ProfScope ps(e, s, PC_ODE, 0);
    HIPCHK(e, launch_cfg_combine(e->dt, p.v32, p.B, (int64_t)p.T * dit->Mp, use_cfg, cfg_strength, kout, nullptr, nullptr, nullptr, 0.f, s));
    dit->last_nfe += 1;
    return ST_OK;
}

int solve_adaptive(st_engine* e, const Plan& p, const float* mask, int use_cfg, float cfg_strength,
                   const RkTableau& tb, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int S = tb.n;
    bool fsal = tb.csol[S] == 0.0;
    for (int j = 0; j < S; ++j) fsal = fsal && tb.csol[j] == tb.beta[S - 1][j];
    const double rtol = 1e-5, atol = 1e-5, t_end = 1.0;
    const int B = p.B;
    const int64_t nstate = (int64_t)B * p.T * dit->Mp;
    const double count = (double)B * dit->M * p.T;            // padded channels carry zeros and do not count
    int rc;
    auto eval = [&](double t, float* kout) { return eval_rhs(e, p, mask, use_cfg, cfg_strength, (float)t, kout, s); };
    float host2[2];
    auto norms = [&](OdeNormArgs a) -> int {
        a.rtol = (float)rtol; a.atol = (float)atol; a.n = nstate; a.partial = p.ode_partial; a.out = p.ode_out;
        HIPCHK(e, launch_ode_norm(a, s));
        HIPCHK(e, hipMemcpyAsync(host2, p.ode_out, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        return ST_OK;
    };
    float* y = p.xstate; float* y1 = p.ynew;
    float* k[7];
    for (int j = 0; j < 7; ++j) k[j] = p.kbuf[j];
    // f0 = f(0, y0)   (x16 already holds y0)
    if ((rc = eval(0.0, k[0]))) return rc;
    // _select_initial_step(order - 1)
    OdeNormArgs na; memset(&na, 0, sizeof(na));
    na.mode = 0; na.y = y; na.b = k[0];
    if ((rc = norms(na))) return rc;
    const double d0 = sqrt(host2[0] / count), d1 = sqrt(host2[1] / count);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    {
        const float* ks[1] = {k[0]}; const float cf[1] = {(float)h0};
        HIPCHK(e, launch_lincomb(e->dt, y, ks, cf, 1, nstate, nullptr, p.x16, p.x16lo, s));
    }
    if ((rc = eval(0.0 + h0, k[1]))) return rc;
    memset(&na, 0, sizeof(na));
    na.mode = 1; na.y = y; na.a = k[0]; na.b = k[1];
    if ((rc = norms(na))) return rc;
    const double d2 = sqrt(host2[0] / count) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3)
                                                   : pow(0.01 / std::max(d1, d2), 1.0 / (double)tb.order);
    double dt = std::min(100.0 * h0, h1), t = 0.0;
    for (int64_t step = 0; step < 1000000; ++step) {
        const double t1 = t + dt;
        for (int i = 0; i < S; ++i) {       // stage i+1: y_i = y + dt * sum_j beta[i][j] k_j ; k_{i+1} = f(t_i, y_i)
            const float* ks[7]; float cf[7]; int nk = 0;
            for (int j = 0; j <= i; ++j) if (tb.beta[i][j] != 0.0) { ks[nk] = k[j]; cf[nk] = (float)(tb.beta[i][j] * dt); ++nk; }
            {
                ProfScope ps(e, s, PC_ODE, 0);
                // with an FSAL tableau (c_sol[:-1] == beta[-1], c_sol[-1] == 0) the last stage input IS y1
                HIPCHK(e, launch_lincomb(e->dt, y, ks, cf, nk, nstate, (fsal && i == S - 1) ? y1 : nullptr, p.x16, p.x16lo, s));
            }
            const double ti = (tb.alpha[i] == 1.0) ? t1 : t + tb.alpha[i] * dt;
            if ((rc = eval(ti, k[i + 1]))) return rc;
        }
        if (!fsal) {                        // y1 = y + dt * sum_j c_sol[j] k_j
            const float* ks[7]; float cf[7]; int nk = 0;
            for (int j = 0; j <= S; ++j) if (tb.csol[j] != 0.0) { ks[nk] = k[j]; cf[nk] = (float)(tb.csol[j] * dt); ++nk; }
            ProfScope ps(e, s, PC_ODE, 0);
            HIPCHK(e, launch_lincomb(e->dt, y, ks, cf, nk, nstate, y1, p.x16, p.x16lo, s));
        }
        // error estimate from the stage derivatives
        memset(&na, 0, sizeof(na));
        na.mode = 2; na.y = y; na.a = y1; na.nk = 0;
        for (int j = 0; j <= S; ++j) if (tb.cerr[j] != 0.0) { na.k[na.nk] = k[j]; na.coef[na.nk] = (float)(tb.cerr[j] * dt); ++na.nk; }
        if ((rc = norms(na))) return rc;
        const double ratio = sqrt(host2[0] / count);
        if (!(ratio == ratio)) return e->fail(ST_ERR_INVALID, std::string(tb.name) + ": non-finite error estimate");
        const bool accept = ratio <= 1.0;
        double dt_next;
        if (ratio == 0.0) dt_next = dt * 10.0;
        else {
            const double dfactor = ratio < 1.0 ? 1.0 : 0.2;
            dt_next = dt * std::min(10.0, std::max(0.9 / pow(ratio, 1.0 / (double)tb.order), dfactor));
        }
        dit->last_steps += 1;
        if (accept) {
            if (t1 >= t_end) {      // dense output at t_end inside [t, t1] -> p.ynew; slot 6 of the kernel is f1 = k[S]
                const float* ks[7]; float cm[7];
                for (int j = 0; j < 7; ++j) { ks[j] = k[0]; cm[j] = 0.f; }
                for (int j = 0; j < S; ++j) { ks[j] = k[j]; cm[j] = (float)(tb.cmid[j] * dt); }
                ks[6] = k[S]; cm[6] = (float)(tb.cmid[S] * dt);
                ProfScope ps(e, s, PC_ODE, 0);
                // elementwise, so writing p.ynew in place is safe whichever of y / y1 it currently aliases
                HIPCHK(e, launch_dopri5_interp(y, y1, ks, cm, (float)dt, (float)((t_end - t) / (t1 - t)), nstate, p.ynew, s));
                return ST_OK;
            }
            std::swap(y, y1);                        // y <- y1
            std::swap(k[0], k[S]);                   // f0 <- k[-1]
            t = t1;
        } else {
            dit->last_rejects += 1;
        }
        dt = dt_next;
        if (!(dt > 0.0) || dt < 1e-12) return e->fail(ST_ERR_INVALID, std::string(tb.name) + ": step size underflow");
    }
    return e->fail(ST_ERR_INVALID, std::string(tb.name) + ": too many steps");
}

// Exact Adams-Bashforth / Adams-Moulton weights for `order` samples on a uniform grid, newest first (bashforth: samples at
// t0, t0 - dt, ...; moulton: t1, t0, t0 - dt, ...), from the integrals of the Lagrange basis over one step.  Long double is
// ample for order <= 12 (the integer tables torchdiffeq stores are these numbers over a common divisor).
static void adams_weights(int order, bool implicit, double* w) {
    std::vector<long double> nodes((size_t)order);
    for (int i = 0; i < order; ++i) nodes[(size_t)i] = implicit ? (i == 0 ? 1.0L : -(long double)(i - 1)) : -(long double)i;
    for (int j = 0; j < order; ++j) {
        std::vector<long double> poly(1, 1.0L);     // prod_{i != j} (u - x_i), lowest degree first
        long double den = 1.0L;
        for (int i = 0; i < order; ++i) {
            if (i == j) continue;
            poly.insert(poly.begin(), 0.0L);
            for (size_t k = 0; k + 1 < poly.size(); ++k) poly[k] -= nodes[(size_t)i] * poly[k + 1];
            den *= nodes[(size_t)j] - nodes[(size_t)i];
        }
        long double integ = 0.0L;
        for (size_t k = 0; k < poly.size(); ++k) integ += poly[k] / (long double)(k + 1);
        w[j] = (double)(integ / den);
    }
}

// torchdiffeq's 'implicit_adams' (fixed_adams.py: AdamsBashforthMoulton, max_order 12, max_iters 4) on the fixed grid of
// models/flow_matching.py:46, rtol = atol = 1e-5 as at :54 -- the eighth solver the reference's web UI offers (webui.py:110).
// Restated from the published source (oracle: odeint_implicit_adams, which says PARITY UNPINNED: torchdiffeq is absent offline).
// Per step: f0 = f(t0, y0) joins the history (newest first, <= 11 entries); fewer than 3 entries -> 3/8-rule Runge-Kutta step
// reusing f0; otherwise Adams-Bashforth predictor over the history, then functional iteration of the Adams-Moulton corrector
// dy <- dt m0 f(t1, y0 + dy) + delta until max |dy_old - dy| / (atol + rtol max(|dy_old|, |dy|)) < 1 (one device reduction and
// an 8-byte read-back per iteration), at most 4 times; no convergence -> the oldest history entry is dropped.
int solve_implicit_adams(st_engine* e, const Plan& p, const float* mask, int use_cfg, float cfg_strength, int n_steps,
                         hipStream_t s) {
    DitState* dit = dit_of(e);
    constexpr int kMaxHist = 11, kMaxIters = 4, kExtra = 11;
    const double rtol = 1e-5, atol = 1e-5;
    const int64_t nstate = (int64_t)p.B * p.T * dit->Mp;
    const size_t sbytes = (size_t)nstate * 4;
    int rc;
    // 19 state-sized fp32 buffers: 11 history + zero + dy x 2 + delta + f / Runge-Kutta stages x 3 + 1 spare; the plan has 8
    if (dit->adams_bytes < sbytes * kExtra) {
        if (dit->adams_buf) { HIPCHK(e, hipStreamSynchronize(s)); hipFree(dit->adams_buf); dit->adams_buf = nullptr; dit->adams_bytes = 0; }
        HIPCHK(e, hipMalloc(&dit->adams_buf, sbytes * kExtra));
        dit->adams_bytes = sbytes * kExtra;
    }
    std::vector<float*> pool;
    for (int j = 0; j < 7; ++j) pool.push_back(p.kbuf[j]);
    pool.push_back(p.ynew);
    for (int j = 0; j < kExtra; ++j) pool.push_back((float*)((char*)dit->adams_buf + (size_t)j * sbytes));
    float* zero = pool.back(); pool.pop_back();
    float* dyA = pool.back(); pool.pop_back();
    float* dyB = pool.back(); pool.pop_back();
    float* delta = pool.back(); pool.pop_back();
    float* tmp[3]; for (int j = 0; j < 3; ++j) { tmp[j] = pool.back(); pool.pop_back(); }
    HIPCHK(e, hipMemsetAsync(zero, 0, sbytes, s));
    std::deque<float*> hist;        // newest first; `pool` holds the free buffers (>= 12 left)
    auto eval = [&](float t, float* kout) { return eval_rhs(e, p, mask, use_cfg, cfg_strength, t, kout, s); };
    // out = base + sum_j cf[j] * ks[j] for any number of terms (lincomb takes 7 at a time); optionally also the operand pair
    auto combine = [&](const float* base, const std::vector<const float*>& ks, const std::vector<float>& cf, float* out32, bool operands) -> int {
        size_t done = 0;
        const float* cur = base;
        do {
            const int nk = (int)std::min<size_t>(7, ks.size() - done);
            const bool last = done + (size_t)nk == ks.size();
            ProfScope ps(e, s, PC_ODE, 0);
            HIPCHK(e, launch_lincomb(e->dt, cur, ks.data() + done, cf.data() + done, nk, nstate, out32,
                                     last && operands ? p.x16 : nullptr, last && operands ? p.x16lo : nullptr, s));
            cur = out32; done += (size_t)nk;
        } while (done < ks.size());
        return ST_OK;
    };
    float* y = p.xstate;
    const std::vector<float> grid = linspace01(n_steps);
    float host2[2];
    for (int i = 0; i < n_steps; ++i) {
        const float t0 = grid[(size_t)i], t1 = grid[(size_t)i + 1], dt = t1 - t0;
        // f0 = f(t0, y)  (x16 holds y); joins the history
        if ((int)hist.size() == kMaxHist) { pool.push_back(hist.back()); hist.pop_back(); }
        float* f0 = pool.back(); pool.pop_back();
        if ((rc = eval(t0, f0))) return rc;
        hist.push_front(f0);
        const int order = (int)hist.size();
        if (order < 3) {        // rk4_alt_step_func with k1 = f0
            if ((rc = combine(y, {f0}, {dt / 3.0f}, nullptr, true))) return rc;
            if ((rc = eval(t0 + dt / 3.0f, tmp[0]))) return rc;
            if ((rc = combine(y, {tmp[0], f0}, {dt, -dt / 3.0f}, nullptr, true))) return rc;
            if ((rc = eval(t0 + dt * 2.0f / 3.0f, tmp[1]))) return rc;
            if ((rc = combine(y, {f0, tmp[0], tmp[1]}, {dt, -dt, dt}, nullptr, true))) return rc;
            if ((rc = eval(t1, tmp[2]))) return rc;
            if ((rc = combine(y, {f0, tmp[0], tmp[1], tmp[2]}, {dt * 0.125f, dt * 0.375f, dt * 0.375f, dt * 0.125f}, y, true))) return rc;
            continue;
        }
        double wb[12], wm[13];
        adams_weights(order, false, wb);
        adams_weights(order + 1, true, wm);
        std::vector<const float*> hs(hist.begin(), hist.end());
        std::vector<float> cb((size_t)order), cm((size_t)order);
        for (int j = 0; j < order; ++j) { cb[(size_t)j] = (float)((double)dt * wb[j]); cm[(size_t)j] = (float)((double)dt * wm[j + 1]); }
        float* dy = dyA; float* dyn = dyB;
        if ((rc = combine(zero, hs, cb, dy, false))) return rc;             // predictor
        if ((rc = combine(zero, hs, cm, delta, false))) return rc;
        bool converged = false;
        for (int it = 0; it < kMaxIters && !converged; ++it) {
            if ((rc = combine(y, {dy}, {1.0f}, nullptr, true))) return rc;      // operands of f(t1, y + dy)
            if ((rc = eval(t1, tmp[0]))) return rc;
            if ((rc = combine(delta, {tmp[0]}, {(float)((double)dt * wm[0])}, dyn, false))) return rc;
            OdeNormArgs na; memset(&na, 0, sizeof(na));
            na.mode = 3; na.y = dy; na.a = dy; na.b = dyn; na.rtol = (float)rtol; na.atol = (float)atol; na.n = nstate;
            na.partial = p.ode_partial; na.out = p.ode_out;
            HIPCHK(e, launch_ode_norm(na, s));
            HIPCHK(e, hipMemcpyAsync(host2, p.ode_out, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(e, hipStreamSynchronize(s));
            converged = host2[0] == 0.0f;
            std::swap(dy, dyn);
        }
        if (!converged) { pool.push_back(hist.back()); hist.pop_back(); dit->last_rejects += 1; }     // (torchdiffeq warns and drops the oldest sample)
        if ((rc = combine(y, {dy}, {1.0f}, y, true))) return rc;            // y1 = y0 + dy, and its operands for the next f0
    }
    return ST_OK;
}

// ---- st_cfm_solve ----------------------------------------------------------------------------
struct Part { Plan p; int b0, nb; hipStream_t s; const float* mask; };

// What the pieces of one st_cfm_solve call share.
struct Solve {
    int B, T, n_steps, solver, use_cfg; float cfg_strength;
    bool adams, adaptive;           // adaptive: host-side controller, one part, eager, time tables per evaluation (incl. implicit Adams)
    int64_t per_item, bct;          // elements per utterance of the state / of a (B, n_feats, T) boundary tensor
    std::vector<Part> parts;
    std::vector<float> dts;         // step sizes of the fixed grid
};

// Utterances are independent ODE solves.  A large fixed-grid batch is solved as TWO (from B = 32 at T = 1000: FOUR) parts
// (contiguous utterance ranges) on as many streams: every kernel of this path alternates an MFMA-bound K loop with an
// HBM-bound epilogue, and with one launch at a time all CUs sit in the same phase (1 block per CU, lock step).
// Two half-size launch sequences, started one evaluation apart, put different kernels / phases on the chip at
// the same time, so the matrix pipes of one part's blocks run under the other part's epilogues.  Results are
// bitwise independent of the split (an utterance never shares a tile with another).  Adaptive solvers keep ONE
// part: their step controller takes the error norm over the whole batch.  ST_SPLIT=0|1|2 overrides (read per call).
int solve_part_count(const st_engine* e, int B, int T, int use_cfg, bool adaptive) {
    const DitState* dit = dit_of(e);
    int nparts = 1;
    const char* sv = getenv("ST_SPLIT");
    const int want = sv ? atoi(sv) : kDefaultSplit;
    const int64_t frames = (int64_t)(use_cfg ? 2 : 1) * B * T;
    if (!adaptive && !e->capture && B >= 2 && (want >= 2 || (want != 0 && want != 1 && frames >= 24000 && B >= 8))) nparts = 2;
    // four parts from 48 000 CFG-doubled frames on (B >= 32 at T = 1000): 25.5 -> 24.8 ms at the headline size, interleaved A/B
    // (profiles/r03_ab_solve_parts.txt); six or eight parts are much slower (31 / 29.5 ms: 40-block launches from 6-8 queues)
    // ... with the generic q/k/v tile.  With the weight-stationary q/k/v kernel (qkv_ws.hip, default) TWO parts are faster: its
    // persistent blocks want >= 5 tiles each, i.e. half-batch launches (paired A/B, round 4: 2 parts + qkv_ws 24.60 ms against
    // 4 parts + generic tile 24.91, ragged 21.61 against 22.09; profiles/r04b_ab_parts_qkv_ws.txt)
    if (!adaptive && !e->capture && want != 0 && want != 1 && want != 2 && frames >= 48000 && B >= 32 && !(dit->qkv_ws && dit->sink)) nparts = 4;
    if (want > 2 && B >= want) nparts = std::min(want, kMaxParts);
    if (want == 1 || want == 0) nparts = 1;
    return nparts;
}

// Boundary conversions into the parts (caller's layouts -> engine operands), on the caller's stream.
int boundary_in(st_engine* e, Solve& sv, const float* mu, const float* mask, const float* z, const float* c, const float* fake_speaker,
                const float* fake_content, const std::vector<float>& tv, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int T = sv.T;
    for (auto& pt : sv.parts) {
        const Plan& p = pt.p;
        ProfScope ps(e, s, PC_PREP, 0);
        HIPCHK(e, launch_set_values(p.tvals, tv.data(), (int)tv.size(), s));   // by kernel argument: no copy, no sync
        HIPCHK(e, launch_mask_prep(mask + (int64_t)pt.b0 * T, pt.nb, T, p.Tp, p.n_full, p.kv_end, p.kbias, p.t_lim, s));
        HIPCHK(e, hipMemsetAsync(p.v32, 0, (size_t)p.N * T * dit->Mp * 4, s));      // frames of skipped tiles: v = 0 (estimator.py:138)
        HIPCHK(e, launch_cvec_prep(mask + (int64_t)pt.b0 * T, nullptr, pt.nb, T, p.maskbuf, s));      // plain copy of the (B,1,T) mask
        pt.mask = p.maskbuf;
        HIPCHK(e, launch_to_time_major(e->dt, mu + pt.b0 * sv.bct, pt.nb, dit->M, T, dit->Mp, nullptr, p.mu16, nullptr, s));
        HIPCHK(e, launch_to_time_major(e->dt, z + pt.b0 * sv.bct, pt.nb, dit->M, T, dit->Mp, p.xstate, p.x16, p.x16lo, s));
        HIPCHK(e, launch_cvec_prep(c + (int64_t)pt.b0 * dit->G, sv.use_cfg ? fake_speaker : nullptr, pt.nb, dit->G, p.cvec, s));
        if (sv.use_cfg) {
            // uncond branch inputs (flow_matching.py:59-60): fake_content over ALL frames, fake_speaker per item
            HIPCHK(e, launch_fill_rows16(e->dt, fake_content, dit->M, dit->Mp, T,
                                         (char*)p.mu16 + (size_t)pt.nb * sv.per_item * 2, s));
        }
    }
    return ST_OK;
}

// One solver step of one part (fixed grid), on the part's stream: estimator evaluation(s) + state update.
int step_fixed(st_engine* e, const Solve& sv, const Part& pt, int i) {
    const Plan& p = pt.p;
    const hipStream_t s = pt.s;
    const int Bp = pt.nb, use_cfg = sv.use_cfg;
    const int64_t per_item = sv.per_item, nstate = (int64_t)Bp * per_item;
    const float cfg_strength = sv.cfg_strength, dt = sv.dts[i];
    int rc;
    if (sv.solver == ST_SOLVER_EULER) {
        if ((rc = run_estimator(e, p, pt.mask, i, s))) return rc;
        ProfScope ps(e, s, PC_ODE, 0);
        HIPCHK(e, launch_cfg_combine(e->dt, p.v32, Bp, per_item, use_cfg, cfg_strength, nullptr, p.xstate, p.x16, p.x16lo, dt, s));
    } else if (sv.solver == ST_SOLVER_MIDPOINT) {
        if ((rc = run_estimator(e, p, pt.mask, 2 * i, s))) return rc;
        {
            ProfScope ps(e, s, PC_ODE, 0);
            HIPCHK(e, launch_cfg_combine(e->dt, p.v32, Bp, per_item, use_cfg, cfg_strength, p.kbuf[0], nullptr, nullptr, nullptr, 0.f, s));
            const float* ks[1] = {p.kbuf[0]}; const float cf[1] = {0.5f * dt};
            HIPCHK(e, launch_lincomb(e->dt, p.xstate, ks, cf, 1, nstate, nullptr, p.x16, p.x16lo, s));
        }
        if ((rc = run_estimator(e, p, pt.mask, 2 * i + 1, s))) return rc;
        ProfScope ps(e, s, PC_ODE, 0);
        HIPCHK(e, launch_cfg_combine(e->dt, p.v32, Bp, per_item, use_cfg, cfg_strength, nullptr, p.xstate, p.x16, p.x16lo, dt, s));
    } else {   // rk4 = torchdiffeq's 3/8 rule
        for (int st = 0; st < 4; ++st) {
            if ((rc = run_estimator(e, p, pt.mask, 4 * i + st, s))) return rc;
            ProfScope ps(e, s, PC_ODE, 0);
            HIPCHK(e, launch_cfg_combine(e->dt, p.v32, Bp, per_item, use_cfg, cfg_strength, p.kbuf[st], nullptr, nullptr, nullptr, 0.f, s));
            if (st == 0) {
                const float* ks[1] = {p.kbuf[0]}; const float cf[1] = {dt / 3.0f};
                HIPCHK(e, launch_lincomb(e->dt, p.xstate, ks, cf, 1, nstate, nullptr, p.x16, p.x16lo, s));
            } else if (st == 1) {
                const float* ks[2] = {p.kbuf[1], p.kbuf[0]}; const float cf[2] = {dt, -dt / 3.0f};
                HIPCHK(e, launch_lincomb(e->dt, p.xstate, ks, cf, 2, nstate, nullptr, p.x16, p.x16lo, s));
            } else if (st == 2) {
                const float* ks[3] = {p.kbuf[0], p.kbuf[1], p.kbuf[2]}; const float cf[3] = {dt, -dt, dt};
                HIPCHK(e, launch_lincomb(e->dt, p.xstate, ks, cf, 3, nstate, nullptr, p.x16, p.x16lo, s));
            } else {
                const float* ks[4] = {p.kbuf[0], p.kbuf[1], p.kbuf[2], p.kbuf[3]};
                const float cf[4] = {dt * 0.125f, dt * 0.375f, dt * 0.375f, dt * 0.125f};
                HIPCHK(e, launch_lincomb(e->dt, p.xstate, ks, cf, 4, nstate, p.xstate, p.x16, p.x16lo, s));
            }
        }
    }
    return ST_OK;
}

// Everything between the boundary conversions touches engine memory only, so for the fixed-grid solvers it is a static launch
// sequence: the body enqueues it, either directly or once into a HIP graph.  Parts 1.. run on the engine's part streams, forked
// from and joined back into `cs` -- on every exit: the guard joins them when an error returns early (before the caller re-zeroes
// the arena they write, and before a capture ends), and the host interleaves the parts step by step, so part k trails part 0.
int solve_body(st_engine* e, Solve& sv, hipStream_t cs) {
    DitState* dit = dit_of(e);
    StreamFork& f = dit->part_streams;
    ForkGuard guard{f, cs};
    const int nparts = (int)sv.parts.size();
    int rc;
    dit->conc = nparts;
    HIPCHK(e, f.fork(cs, nparts - 1));
    for (int k = 0; k < nparts; ++k) sv.parts[k].s = k == 0 ? cs : f.child[k - 1];
    for (auto& pt : sv.parts) {
        if ((rc = run_prenet(e, pt.p, pt.s))) return rc;
        if ((rc = run_adaln(e, pt.p, pt.s))) return rc;
        if (!sv.adaptive && (rc = run_time_tables(e, pt.p, pt.s))) return rc;
    }
    if (sv.adams) {
        if ((rc = solve_implicit_adams(e, sv.parts[0].p, sv.parts[0].mask, sv.use_cfg, sv.cfg_strength, sv.n_steps, cs))) return rc;
    } else if (sv.adaptive) {
        const RkTableau& tb = sv.solver == ST_SOLVER_BOSH3 ? kBosh3 : sv.solver == ST_SOLVER_FEHLBERG2 ? kFehlberg2
                            : sv.solver == ST_SOLVER_ADAPTIVE_HEUN ? kAdaptiveHeun : kDopri5;
        if ((rc = solve_adaptive(e, sv.parts[0].p, sv.parts[0].mask, sv.use_cfg, sv.cfg_strength, tb, cs))) return rc;
    } else {
        // The parts run the same kernel sequence; started together they tend to sit in the same kernel at the same time (FFN beside
        // FFN: two power-limited kernels sharing the CUs).  Part k starts 100 k us late -- about half a layer of a half batch: any
        // offset from 30 to 250 us measured +0.4 ... +0.6 % per solve, paired (profiles/r05_ab_part_phase.txt).
        // (Measured for TWO parts at the headline size only: other part counts -- ST_SPLIT=3, 4 -- start together.)
        if (nparts == 2) HIPCHK(e, launch_delay(kPartPhaseUs, sv.parts[1].s));
        for (int i = 0; i < sv.n_steps; ++i)
            for (auto& pt : sv.parts)
                if ((rc = step_fixed(e, sv, pt, i))) return rc;
    }
    HIPCHK(e, f.join(cs));
    return ST_OK;
}

// ST_HIP_GRAPH=1 (read per call): the fixed-grid solve body (~45 launches per evaluation) is captured into a HIP graph the second
// time a solve signature is seen (the first run is eager: it also performs the one-time per-kernel attribute set-up, which must
// not happen inside a capture) and replayed afterwards.  Adaptive solvers have a host-side controller and always run eagerly; so
// do profiled / debug-captured solves.  Sets *replayed when the graph ran the body on `s` (else the caller runs it eagerly).
int solve_graph(st_engine* e, Solve& sv, hipStream_t s, bool* replayed) {
    DitState* dit = dit_of(e);
    const char* genv = getenv("ST_HIP_GRAPH");
    if (!(genv && atoi(genv) == 1 && !sv.adaptive && !e->prof && !e->capture)) return ST_OK;
    const int nparts = (int)sv.parts.size();
    DitState::SolveGraph* g = nullptr;
    for (auto& q : dit->graphs)
        if (q.B == sv.B && q.T == sv.T && q.n_steps == sv.n_steps && q.solver == sv.solver && q.use_cfg == (sv.use_cfg != 0) &&
            q.cfg_strength == sv.cfg_strength && q.ws == e->ws && q.parts == nparts) g = &q;
    if (!g) {
        if (dit->graphs.size() >= 16) dit->drop_graphs();
        dit->graphs.push_back({sv.B, sv.T, sv.n_steps, sv.solver, sv.use_cfg != 0, sv.cfg_strength, e->ws, nparts, 0, nullptr});
        g = &dit->graphs.back();
    }
    if (g->seen >= 1 && !g->exec) {
        // captured on an engine-owned stream (the caller's may be the legacy default stream, which cannot
        // capture); nothing executes during capture, the instantiated graph is launched on the caller's stream
        if (!dit->gstream) HIPCHK(e, hipStreamCreateWithFlags(&dit->gstream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        HIPCHK(e, hipStreamBeginCapture(dit->gstream, hipStreamCaptureModeRelaxed));
        const int brc = solve_body(e, sv, dit->gstream);      // (its part streams are joined back into the capture stream on every exit)
        const hipError_t ec = hipStreamEndCapture(dit->gstream, &graph);
        dit->conc = 1;
        if (brc) { if (graph) hipGraphDestroy(graph); return brc; }
        if (ec != hipSuccess || !graph) return e->fail(ST_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
        const hipError_t ei = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (ei != hipSuccess) { g->exec = nullptr; return e->fail(ST_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
    }
    g->seen += 1;
    if (g->exec) { HIPCHK(e, hipGraphLaunch(g->exec, s)); *replayed = true; }
    return ST_OK;
}

}  // namespace
}  // namespace sthost

using namespace sthost;

extern "C" int st_cfm_solve(st_engine* e, const float* mu, const float* mask, const float* z, const float* c,
                            int n_steps, int solver, int use_cfg, float cfg_strength,
                            const float* fake_speaker, const float* fake_content,
                            float* out, int B, int T, void* stream) {
    int rc = check_ready(e, KIND_DECODER, B, T); if (rc) return rc;
    DitState* dit = dit_of(e);
    if (!mu || !mask || !z || !c || !out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (n_steps < 1 || n_steps > 4096) return e->fail(ST_ERR_INVALID, "n_steps out of range");
    if (solver < ST_SOLVER_EULER || solver > ST_SOLVER_IMPLICIT_ADAMS)
        return e->fail(ST_ERR_UNSUPPORTED, "solver not implemented natively (euler, midpoint, rk4, dopri5, bosh3, "
                                           "fehlberg2, adaptive_heun, implicit_adams are)");
    if (use_cfg && (!fake_speaker || !fake_content)) return e->fail(ST_ERR_INVALID, "CFG needs fake_speaker and fake_content");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const bool adams = solver == ST_SOLVER_IMPLICIT_ADAMS;
    const bool adaptive = solver >= ST_SOLVER_DOPRI5;
    const int stages = solver == ST_SOLVER_EULER ? 1 : (solver == ST_SOLVER_MIDPOINT ? 2 : 4);
    const int n_t = adaptive ? 1 : n_steps * stages;
    const int nparts = solve_part_count(e, B, T, use_cfg, adaptive);
    Solve sv{B, T, n_steps, solver, use_cfg, cfg_strength, adams, adaptive, (int64_t)T * dit->Mp, (int64_t)dit->M * T,
             std::vector<Part>((size_t)nparts), std::vector<float>((size_t)n_steps)};
    {
        size_t off = 0;
        for (int k = 0; k < nparts; ++k) {
            sv.parts[k].b0 = (int)((int64_t)B * k / nparts);
            sv.parts[k].nb = (int)((int64_t)B * (k + 1) / nparts) - sv.parts[k].b0;
            off = layout_plan(e, sv.parts[k].nb, T, use_cfg != 0, n_t, off, &sv.parts[k].p);
        }
        if ((rc = ensure_ws(e, off))) return rc;
        dit->arena_poisoned(e);
        if ((rc = arena_fresh(e, layout_sig(2, B, T, use_cfg != 0, n_t, nparts), off, s))) return rc;
        for (auto& pt : sv.parts) bind_plan(e, &pt.p);
    }
    if ((rc = ensure_rope(e, T, s))) return rc;
    if (nparts > 1) HIPCHK(e, dit->part_streams.ensure(nparts - 1, 1, 0));

    // evaluation times, fp32 arithmetic as torchdiffeq does on the fp32 t_span (flow_matching.py:46)
    const std::vector<float> grid = linspace01(n_steps);
    std::vector<float> tv((size_t)n_t);
    for (int i = 0; i < n_steps && !adaptive; ++i) {
        const float t0 = grid[i], t1 = grid[i + 1], dt = t1 - t0;
        sv.dts[i] = dt;
        if (stages == 1) tv[i] = t0;
        else if (stages == 2) { tv[2 * i] = t0; tv[2 * i + 1] = t0 + 0.5f * dt; }
        else { tv[4 * i] = t0; tv[4 * i + 1] = t0 + dt / 3.0f; tv[4 * i + 2] = t0 + dt * 2.0f / 3.0f; tv[4 * i + 3] = t1; }
    }
    if ((rc = boundary_in(e, sv, mu, mask, z, c, fake_speaker, fake_content, tv, s))) return rc;
    dit->last_nfe = adaptive ? 0 : (int64_t)n_t; dit->last_steps = adaptive && !adams ? 0 : n_steps; dit->last_rejects = 0;

    bool replayed = false;
    if ((rc = solve_graph(e, sv, s, &replayed))) return rc;
    if (!replayed) {
        rc = solve_body(e, sv, s);      // (returns with its part streams joined into s)
        dit->conc = 1;
        if (rc) { e->ws_sig = 0; return rc; }      // (a half-enqueued body: re-zero the arena next time)
    }
    for (auto& pt : sv.parts) {      // boundary conversion of the result
        ProfScope ps(e, s, PC_PREP, 0);
        HIPCHK(e, launch_from_time_major(adaptive && !adams ? pt.p.ynew : pt.p.xstate, pt.nb, dit->M, T, dit->Mp, out + pt.b0 * sv.bct, s, dit->status_dev));
    }
    return ST_OK;
}
