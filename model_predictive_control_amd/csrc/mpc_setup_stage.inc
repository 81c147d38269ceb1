// mpc_setup_stage.inc -- one trip of the setup loop of mpc_group_kernel
// (quad_box.hip): x-bar stage t next to Riccati stage k = N-1-t, and in row
// form the columns of stage k of W~ and the Lyapunov recursion for f.  Plain
// text, included once per combination of the wave-uniform launch flags:
//   MPCQP_STAGE_TV  time-varying plant (the stage's A, B are read from LDS)
//   MPCQP_STAGE_HC  a drift c is present
// either the kernel's run-time values (one loop that tests them in every
// stage) or literals (MPCQP_SETUP_UNIFORM: one loop per combination, chosen
// in front of it).  A lambda or a helper template in its place changes the
// instruction streams of the kernels that keep the run-time flags.
{
  {  // x-bar stage t: x_{t+1} = A_t x_t + c_t
    if (MPCQP_STAGE_TV) load_sq<T, NX, NX>(As + t * NX * NX, Ax, NX);
    T xn[NX], cs[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) cs[i] = T(0);
    if constexpr (C_AHEAD) {
#pragma unroll
      for (int i = 0; i < NX; ++i) cs[i] = ct[i];
      if (MPCQP_STAGE_HC) {
        const int tn = t + 1 < N ? t + 1 : t;
#pragma unroll
        for (int i = 0; i < NX; ++i) ct[i] = Cs[tn * NX + i];
      }
    } else if (MPCQP_STAGE_HC) {
#pragma unroll
      for (int i = 0; i < NX; ++i) cs[i] = Cs[t * NX + i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      T s = cs[i];
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) s = fma(Ax[i][qq], xk[qq], s);
      xn[i] = s;
    }
#pragma unroll
    for (int qq = 0; qq < NX; ++qq) xk[qq] = xn[qq];
    if constexpr (ROWS) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) xr[ch][qq] = t == rt[ch] ? xk[qq] : xr[ch][qq];
    } else if (q == 0) {
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) Xs[(t + 1) * NX + qq] = xk[qq];
    }
  }
  const int k = N - 1 - t;
  if (MPCQP_STAGE_TV) {
    load_sq<T, NX, NX>(As + k * NX * NX, Ar, NX);
    load_sq<T, NX, NU>(Bs + k * NX * NU, Br, NU);
  }
  T PA[NX][NX], PB[NX][NU];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      T s = T(0);
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) s = fma(P[i][qq], Ar[qq][j], s);
      PA[i][j] = s;
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      T s = T(0);
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) s = fma(P[i][qq], Br[qq][j], s);
      PB[i][j] = s;
    }
  }
  T Sm[NU][NU], Y[NU][NX];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      T s = Rr[i][j];
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) s = fma(Br[qq][i], PB[qq][j], s);
      Sm[i][j] = s;
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      T s = T(0);
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) s = fma(Br[qq][i], PA[qq][j], s);
      Y[i][j] = s;
    }
  }
  T Si[NU][NU];
  [[maybe_unused]] const T s00 = Sm[0][0];
  // S^{-1} by Gauss-Jordan (S symmetric positive definite)
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int j = 0; j < NU; ++j) Si[i][j] = (i == j) ? T(1) : T(0);
#pragma unroll
  for (int p = 0; p < NU; ++p) {
    ok &= Sm[p][p] > T(0);
    const T rp = T(1) / Sm[p][p];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      Sm[p][j] *= rp;
      Si[p][j] *= rp;
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if (i == p) continue;
      const T fct = Sm[i][p];
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        Sm[i][j] = fma(-fct, Sm[p][j], Sm[i][j]);
        Si[i][j] = fma(-fct, Si[p][j], Si[i][j]);
      }
    }
  }
  T K[NU][NX];
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      T s = T(0);
#pragma unroll
      for (int qq = 0; qq < NU; ++qq) s = fma(Si[i][qq], Y[qq][j], s);
      K[i][j] = -s;
    }
  if constexpr (!ROWS) {
    // two-loop setup: K_k, S_k^-1 and A_k + B_k K_k for the second loop
    if (q == 0) {
#pragma unroll
      for (int i = 0; i < NU; ++i) {
#pragma unroll
        for (int j = 0; j < NX; ++j) Ks[(k * NU + i) * NX + j] = K[i][j];
#pragma unroll
        for (int j = 0; j < NU; ++j) Sis[(k * NU + i) * NU + j] = Si[i][j];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          T s = Ar[i][j];
#pragma unroll
          for (int qq = 0; qq < NU; ++qq) s = fma(Br[i][qq], K[qq][j], s);
          Acls[(k * NX + i) * NX + j] = s;
        }
    }
  } else {
    // row form: columns (k, :) of W~, the rows of every lane; then
    // Psi_{k-1} (mpc_factor.hpp)
    T Acl[NX][NX], Lk[NU][NU];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        T s = Ar[i][j];
#pragma unroll
        for (int qq = 0; qq < NU; ++qq) s = fma(Br[i][qq], K[qq][j], s);
        Acl[i][j] = s;
      }
    chol_lower<T, NU>(s00, Si, Lk);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const bool at = k == rt[ch];
      // v = e_a' at the row's own stage, Psi_k(rt)[a, :] B_k after it.  The
      // rows of earlier stages (rt < k) and the padding rows n .. NV-1
      // store 0 * B_k * L_k, which is 0 only while those are finite: in
      // the NOT_CONVEX case (NaN or Inf in L_k, K_k) the tile holds NaN
      // there, which nothing uses -- gi_box runs only with code ==
      // OPTIMAL and z is overwritten with NaN.
      T v[NU], w[NU];
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        T s = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(psi[ch][qq], Br[qq][i], s);
        v[i] = at ? (ra1[ch] == (i == 1) ? T(1) : T(0)) : s;
      }
      // w = v L_k (L_k lower triangular)
#pragma unroll
      for (int bb = 0; bb < NU; ++bb) {
        T s = v[bb] * Lk[bb][bb];
#pragma unroll
        for (int i = bb + 1; i < NU; ++i) s = fma(v[i], Lk[i][bb], s);
        w[bb] = s;
      }
      if (q + ch * GL < NV) {
#pragma unroll
        for (int bb = 0; bb < NU; ++bb)
          if (bb < nu) Wt[(k * nu + bb) * ld + q + ch * GL] = w[bb];
      }
      T pn[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        T s = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(psi[ch][qq], Acl[qq][j], s);
        pn[j] = at ? (ra1[ch] ? K[NU - 1][j] : K[0][j]) : s;
      }
#pragma unroll
      for (int j = 0; j < NX; ++j) psi[ch][j] = pn[j];
    }
    // g_k = B_k' Pi_{k+1}, h_k = B_k' pi_{k+1}, caught by the rows of stage
    // k; then Pi_k = Q + A_k' Pi_{k+1} A_k, pi_k = A_k'(Pi_{k+1} c_k + pi_{k+1})
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      T gu[NX];
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        T s = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(Br[qq][u], Pi[qq][j], s);
        gu[j] = s;
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const bool mine = k == rt[ch] && ra1[ch] == (u == 1);
#pragma unroll
        for (int j = 0; j < NX; ++j) gr[ch][j] = mine ? gu[j] : gr[ch][j];
      }
      if (MPCQP_STAGE_HC) {
        T hu = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) hu = fma(Br[qq][u], pv[qq], hu);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          hr[ch] = (k == rt[ch] && ra1[ch] == (u == 1)) ? hu : hr[ch];
      }
    }
    // (also at k = 0, where the results are not used: without the branch
    // the loop carries no copies of Pi and P)
    {
      if (MPCQP_STAGE_HC) {
        T tmp[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          T s = pv[i];
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) s = fma(Pi[i][qq], Cs[k * NX + qq], s);
          tmp[i] = s;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          T s = T(0);
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) s = fma(Ar[qq][i], tmp[qq], s);
          pv[i] = s;
        }
      }
      T PiA[NX][NX];
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          T s = T(0);
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) s = fma(Pi[i][qq], Ar[qq][j], s);
          PiA[i][j] = s;
        }
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          T s = Qr[i][j];
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) s = fma(Ar[qq][i], PiA[qq][j], s);
          Pi[i][j] = s;
        }
    }
  }
  if (ROWS || k > 0) {
    // P <- Q + A'PA + (A'PB) K
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        T s = Qr[i][j];
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(Ar[qq][i], PA[qq][j], s);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          T apb = T(0);
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) apb = fma(Ar[qq][i], PB[qq][u], apb);
          s = fma(apb, K[u][j], s);
        }
        P[i][j] = s;
      }
  }
}
