// gi_box_trip.inc -- the trip of gi_box_st (gi_box_core.hpp) behind the pivot
// column: ratio test, step, state change, scan-ahead and what the sweep needs.
// One body, included once per path with MPCQP_TRIP_FULL defined:
//   false  the general trip;
//   true   no group of the wave can take a partial step (the ratio filter):
//          partial is the constant false and with it idx = p, sigma = -1 and
//          the sweep column the pivot's; no ratio test, no second publish;
//          with Own::FULL_SWEEP the path's own sweep on them, at its end.
// Per group the arithmetic of a full step is the same on both, in the same
// order.  Plain text and not a lambda or a helper template: either changes the
// registers and the instruction streams of the kernels that have only the
// general trip (an always-inline lambda: all 16 box_gi_kernel instantiations).
{
  constexpr bool FULL = MPCQP_TRIP_FULL;
  T ti = T(0);
  int k = 0;
  if (!FULL) {
    if constexpr (Own::RATE_ONCE) sel.ratio(st, mu, dmu, ti, k);
    else sel.ratio(st, mu, co, rm, sgn, ti, k);
  }
  const bool partial = !FULL && ti < t2;
  const T s_eff = stepping ? (partial ? ti : t2) : T(0);
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    const T cs = co[r] * rm;  // dz per unit move of z_p (c stays raw for the sweep)
    zr[r] = (st[r] == 0) ? fma(sgn * s_eff, cs, zr[r]) : zr[r];
    if constexpr (Own::RATE_ONCE) mu[r] = fma(s_eff, dmu[r], mu[r]);
    else mu[r] = fma(s_eff, mu_rate(st[r], cs, sgn), mu[r]);
  }
  gp = fma(-sgn * s_eff, rm, gp);  // d g_p / d z_p = -1 / M_pp
  zp = fma(sgn, s_eff, zp);
  MPCQP_PHASE(6);
  // the index whose state changes: k joins F (partial) or p leaves it (full)
  const int idx = partial ? k : p;
  const T sigma = partial ? T(1) : T(-1);
  // full steps sweep on p, whose column is still in registers: publish
  // again only when some group of the wave drops a bound
  T kr[BS], kcol[NC];
  T d = mpp;
  if (!FULL && __any(stepping && partial)) {
    d = M.column(idx, gb, kr, kcol);
  } else {
#pragma unroll
    for (int r = 0; r < BS; ++r) kr[r] = c[r];
#pragma unroll
    for (int r = 0; r < NC; ++r) kcol[r] = cc[r];
  }
  const bool bad = stepping && (partial ? !(d > T(0)) : !(d < T(0)));
  // the state changes first, then the next pivot's scan: it reads only z
  // and the states, so its arg-max chain runs ahead of (and can overlap)
  // the sweep; used when the step was full (need_p)
  if (stepping && !bad) {
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const int i = ri[r];
      if (partial && i == k) {
        st[r] = 0;
        mu[r] = T(0);
      }
      if (!partial && i == p) {
        st[r] = side;
        zr[r] = tgt;
        mu[r] = (side == 1) ? gp : -gp;
      }
    }
    need_p = !partial;
  }
  if (bad) {
    code = MPCQP_STATUS_NOT_CONVEX;
    active = false;
  }
  sel.publish(M, zr);
  sel.scan(st, zr, B, a_viol, a_pi, a_zv);
  have_scan = true;
  if constexpr (Own::AHEAD) {
    // The next pivot's bounds and z_p, issued here so that the round
    // trip runs under the sweep.  This trip's publish precedes the read
    // and nothing writes zs before the next one; a group that keeps its
    // pivot ignores the values.  Without a candidate a_pi is the
    // sentinel's index, which may lie past the vectors: clamped.
    const int pa = a_pi < BoxLds<Mat>::NV - 1 ? a_pi : BoxLds<Mat>::NV - 1;
    a_lb = lbs[pa];
    a_ub = ubs[pa];
    a_zp = sel.pivot_z(pa, a_zv);
  }
  if constexpr (Own::FULL_SWEEP && FULL) {
    if (stepping && !bad) M.template sweep_col<true, true>(p, T(-1), rm, c, cc);
  } else if constexpr (Own::FAST) {
    sweeping = stepping && !bad;
    s_idx = idx;
    s_sigma = sigma;
#pragma unroll
    for (int r = 0; r < BS; ++r) s_kr[r] = kr[r];
#pragma unroll
    for (int r = 0; r < NC; ++r) s_kcol[r] = kcol[r];
    // (SWEEP_RD: 1 / d; of a full step that is the trip's rm: same input,
    // same function, same bits)
    s_d = !Own::SWEEP_RD ? d : (FULL ? rm : fast_rcp(d));
  } else {
    if (stepping && !bad) M.sweep_col(idx, sigma, d, kr, kcol);
  }
}
