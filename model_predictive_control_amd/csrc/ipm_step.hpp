// ipm_step.hpp -- the algebra of ONE bounded component v in [lo, hi] with its
// bound duals (ll at lo, lu at hi) in the interior point of ipm_lane.hpp, and
// the control of its iteration.  Scalars in, scalars out, host and device:
// solve_lane / polish (ipm_lane.hpp, per component j inside their stage
// loops), solve_quad / polish_q (ipm_quad.hpp) and solve_wave / polish_w
// (ipm_wave.hpp) all call these, so a formula, a tolerance or the inertia
// schedule stands here once.  An infinite bound has no dual and no term.
// Accumulators (sums and maxima over the components) are passed by reference
// so every caller adds its terms in the order it always did.
#pragma once

#include <cmath>

#include "../../include/mpcqp.h"  // MPCQP_STATUS_*

#ifndef MPCQP_HD
#error "define MPCQP_HD before including ipm_step.hpp"
#endif

#define MPCQP_IL MPCQP_HD inline __attribute__((always_inline))

namespace mpcqp {
namespace ipm {

constexpr double kInf = __builtin_huge_val();

MPCQP_IL bool fin(double v) { return __builtin_isfinite(v); }

// ---------------------------------------------------------- one iteration
// Pass 1: apply the corrector step of the previous iteration.  dv is the
// corrector direction of v, dva the predictor's; the dual directions are
// rebuilt from them (they are never stored).
MPCQP_IL void apply_step(double& v, double& ll, double& lu, double lo, double hi, double dv,
                         double dva, double alpha, double sigmu) {
  if (fin(lo)) {
    const double sl = v - lo;
    const double dla = -ll * (1.0 + dva / sl);
    const double rc = sigmu - sl * ll - dva * dla;
    ll += alpha * ((rc - ll * dv) / sl);
  }
  if (fin(hi)) {
    const double su = hi - v;
    const double dua = -lu * (1.0 - dva / su);
    const double rc = sigmu - su * lu + dva * dua;
    lu += alpha * ((rc + lu * dv) / su);
  }
  v += alpha * dv;
}

// Pass 1: from the gradient g without the bound duals, the stationarity
// residual (-> rstat, a maximum) and the complementarity (-> musum); returns
// Sigma = ll / (v - lo) + lu / (hi - v).
MPCQP_IL double residual_sigma(double v, double ll, double lu, double lo, double hi, double g,
                               double& rstat, double& musum) {
  double sig = 0.0, r = g;
  if (fin(lo)) {
    const double sl = v - lo;
    sig += ll / sl;
    musum += sl * ll;
    r -= ll;
  }
  if (fin(hi)) {
    const double su = hi - v;
    sig += lu / su;
    musum += su * lu;
    r += lu;
  }
  rstat = fmax(rstat, fabs(r));
  return sig;
}

// Pass 2: the predictor direction dv of v: its step to the boundary (-> amax)
// and the affine complementarity (s + a ds)(l + a dl) summed as the quadratic
// c0 + a c1 + a^2 c2.
MPCQP_IL void predictor_terms(double v, double dv, double lo, double hi, double l, double lu,
                              double& amax, double& c0, double& c1, double& c2) {
  if (fin(lo)) {
    const double sl = v - lo;
    const double dl = -l * (1.0 + dv / sl);
    if (dv < 0.0) amax = fmin(amax, -sl / dv);
    if (dl < 0.0) amax = fmin(amax, -l / dl);
    c0 += sl * l;
    c1 += sl * dl + l * dv;
    c2 += dv * dl;
  }
  if (fin(hi)) {
    const double su = hi - v;
    const double dl = -lu * (1.0 - dv / su);
    if (dv > 0.0) amax = fmin(amax, su / dv);
    if (dl < 0.0) amax = fmin(amax, -lu / dl);
    c0 += su * lu;
    c1 += su * dl - lu * dv;
    c2 -= dv * dl;
  }
}

// sigma * mu of the corrector (Mehrotra: sigma = (mu_aff / mu)^3) from the
// predictor's sums over all mcount finite bounds; 0 without bounds.
MPCQP_IL double centering(double mcount, double c0, double c1, double c2, double amax,
                          double mu) {
  if (!(mcount > 0.0)) return 0.0;
  const double mua = (c0 + amax * (c1 + amax * c2)) / mcount;
  const double r = fmax(0.0, fmin(1.0, mua / mu));
  return r * r * r * mu;
}

// Pass 3: the corrector's right-hand side of v: g plus the bound terms with
// the predictor's second-order part.
MPCQP_IL double corrector_rhs(double v, double dva, double lo, double hi, double l, double lu,
                              double g, double sigmu) {
  double s = g;
  if (fin(lo)) {
    const double sl = v - lo;
    s += (-sigmu - dva * l * (1.0 + dva / sl)) / sl;
  }
  if (fin(hi)) {
    const double su = hi - v;
    s += (sigmu - dva * lu * (1.0 - dva / su)) / su;
  }
  return s;
}

// Pass 4: the corrector direction dv of v: its step to the boundary (-> amax).
MPCQP_IL void corrector_bound(double v, double dv, double dva, double lo, double hi, double l,
                              double lu, double sigmu, double& amax) {
  if (fin(lo)) {
    const double sl = v - lo;
    const double dla = -l * (1.0 + dva / sl);
    const double dl = (sigmu - sl * l - dva * dla - l * dv) / sl;
    if (dv < 0.0) amax = fmin(amax, -sl / dv);
    if (dl < 0.0) amax = fmin(amax, -l / dl);
  }
  if (fin(hi)) {
    const double su = hi - v;
    const double dua = -lu * (1.0 - dva / su);
    const double dl = (sigmu - su * lu + dva * dua + lu * dv) / su;
    if (dv > 0.0) amax = fmin(amax, su / dv);
    if (dl < 0.0) amax = fmin(amax, -lu / dl);
  }
}

// ------------------------------------------------------------------ polish
// Tolerance of the polish's tests, relative to 1 + |x|.
MPCQP_IL double polish_tol(double x) { return 1e-9 * (1.0 + fabs(x)); }

// The active-set guess from the interior-point iterate (dual > slack): act =
// +1 at hi, -1 at lo, 0 inactive; y the starting multiplier (> 0 at hi).
MPCQP_IL void polish_guess(double v, double lo, double hi, double l, double u, double& act,
                           double& y) {
  const double rl = fin(lo) ? l / (v - lo) : 0.0;
  const double ru = fin(hi) ? u / (hi - v) : 0.0;
  act = (ru > 1.0 && ru >= rl) ? 1.0 : ((rl > 1.0) ? -1.0 : 0.0);
  y = act > 0.0 ? u : (act < 0.0 ? -l : 0.0);
}

// The penalty of an active component: true with pen = y + rho (v - bound),
// its gradient term (its curvature is rho); false when inactive.
MPCQP_IL bool polish_penalty(double act, double y, double rho, double v, double lo, double hi,
                             double& pen) {
  if (act == 0.0) return false;
  pen = y + rho * (v - (act > 0.0 ? hi : lo));
  return true;
}

// After a step to v: the multiplier update of an active component (act, y:
// its flag and multiplier, updated in place) and the tests.  last (the final
// step of a round): an active component off its bound fails the round (good),
// one with a wrong-sign multiplier is released and an inactive one outside its
// box is added at the violated side (changed).  probe (an earlier step, the
// early exit of the quad and wave polish): the same tests only clear pass.
MPCQP_IL void polish_update(double v, double lo, double hi, double rho, bool last, bool probe,
                            double& act, double& y, bool& good, bool& changed, bool& pass) {
  const double a = act;
  if (a != 0.0) {
    const double bnd = a > 0.0 ? hi : lo;
    const double yn = y + rho * (v - bnd);
    y = yn;
    const bool on = fabs(v - bnd) <= polish_tol(bnd);
    const bool wrong = a > 0.0 ? yn < -polish_tol(yn) : yn > polish_tol(yn);
    if (probe) pass = pass && on && !wrong;
    if (last) {
      good = good && on;
      if (wrong) {  // wrong sign: release
        act = 0.0;
        y = 0.0;
        changed = true;
      }
    }
  } else if (last || probe) {
    const double jl = (lo - v) / (1.0 + fabs(lo));
    const double jh = (v - hi) / (1.0 + fabs(hi));
    if (jl > 1e-9 || jh > 1e-9) {  // violated: fix at the violated side
      if (last) {
        act = jl > jh ? -1.0 : 1.0;
        changed = true;
      }
      pass = false;
    }
  }
}

// --------------------------------------------------------------- iteration
// State of the iteration between its passes.
struct Control {
  double alpha = 0.0, sigmu = 0.0;  // step and sigma*mu of the last corrector
  double mu_pol = 0.0;              // next polish attempt below this mu
  // inertia correction (only a non-convex H2 needs it): on a non-positive
  // pivot pass 1 runs again with a growing dreg; each iteration starts a third
  // below the last one that worked (0 once it falls below 1e-12).  It changes
  // the Newton direction, not the residuals, so the iterate still converges
  // to a KKT point of the QP.  Strict mode (an SQP's QP, whose caller can
  // damp the Hessian instead) gives up after `strict` corrections: a QP that
  // is non-convex only away from its active face needs a few while the
  // barrier terms of the active bounds grow; one that keeps needing them is
  // handed back to the caller.
  double dreg = 0.0, dlast = 0.0;
  int ncorr = 0;
  bool conv = false;  // the last pass 1 met tol / tol_mu
  int code = 0;       // status of a kStop
};

// What follows pass 1 / a failed polish
enum Next : int {
  kStop,    // emit the interior-point iterate with Control::code
  kAgain,   // pass 1 again (alpha = 0: the pending step is applied already)
  kPolish,  // try the polish
  kStep     // passes 2-4
};

template <class A>
MPCQP_IL Next stop_or(Control& c, const A& a, int it, Next next) {
  if (!c.conv && it < a.max_iter) return next;
  c.code = c.conv ? MPCQP_STATUS_OPTIMAL : MPCQP_STATUS_MAXITER;
  return kStop;
}

// The decisions after the factorisation of iteration it: residuals rstat,
// rdyn, mean complementarity mu over the finite bounds (bounded: there are
// any), pd: every pivot was positive.
template <class A>
MPCQP_IL Next after_factor(Control& c, const A& a, int it, bool pd, double rstat, double rdyn,
                           double mu, bool bounded) {
  if (!fin(rstat) || !fin(rdyn) || !fin(mu)) {
    c.code = MPCQP_STATUS_NONFINITE;
    return kStop;
  }
  double& dreg = c.dreg;
  if (!pd) {
    dreg = dreg > 0.0 ? 8.0 * dreg : (c.dlast > 0.0 ? c.dlast : 1e-4);
    if ((a.strict > 0 && ++c.ncorr > a.strict) || dreg > 1e12 || it >= a.max_iter) {
      c.code = MPCQP_STATUS_NOT_CONVEX;
      return kStop;
    }
    c.alpha = 0.0;
    return kAgain;
  }
  if (dreg > 0.0) {  // next iteration starts a third lower
    c.dlast = dreg;
    dreg = dreg / 3.0 > 1e-12 ? dreg / 3.0 : 0.0;
  }
  c.conv = rstat <= a.tol && rdyn <= a.tol && mu <= a.tol_mu;
  if (bounded && c.mu_pol > 0.0 && mu <= c.mu_pol && rstat <= a.tol_polish &&
      rdyn <= a.tol_polish)
    return kPolish;
  return stop_or(c, a, it, kStep);
}

// A polish that did not certify its vertex (wrong active-set guess): keep
// iterating, try again at a smaller mu; the polish overwrote the
// factorisation, so pass 1 runs again.
template <class A>
MPCQP_IL Next after_failed_polish(Control& c, const A& a, int it) {
  c.mu_pol *= 1e-2;
  c.alpha = 0.0;
  return stop_or(c, a, it, kAgain);
}

// Fraction to the boundary.  Fixed, not tightened towards 1 as mu -> 0: the
// slacks are differences v - lo, and a slack driven below the rounding of v
// would turn Sigma = lam / s into inf.
MPCQP_IL double step_length(double amax) { return fmin(1.0, 0.995 * amax); }

}  // namespace ipm
}  // namespace mpcqp
