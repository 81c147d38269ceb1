// ipm_wave.hpp -- the interior point of ipm_quad.hpp (solve_quad) for one
// instance on a WHOLE wavefront: the one-launch SQP (sqp_solve.hip) runs each
// instance in its own single-wave workgroup, where solve_quad kept 60 of the
// 64 lanes idle while one quad walked the horizon four times per iteration.
// Here only the serial chains stay serial, behind three functions (factor,
// forward, rhs: on the fp64 matrix cores, or with -DMPCQP_RICCATI_QUAD on
// quad 0 with solve_quad's helpers):
//   pass 1  the Riccati factorisation,
//   pass 2  the predictor's forward sweep (dx+ = (A + B K) dx + B k + e),
//   pass 3  the corrector's backward right-hand side (p, Pe, h, k, the cost-to-go),
//   pass 4  the corrector's forward sweep,
// and everything per stage runs one quad per stage on the 16 quads of the wave
// before or after its chain: applying the previous step, the dynamics residual,
// the gradients, Sigma and the complementarity of pass 1; the input direction,
// the step to the boundary and the affine complementarity of pass 2; the
// corrector right-hand side of pass 3; the costate direction and the step to
// the boundary of pass 4.  Each of these is the function solve_quad calls for
// the stage (ipm_quad.hpp: pass1..4_stage_q, polish_*_q), and the decisions
// between the passes are ipm_step.hpp's, so the iterates agree with
// solve_quad's to the summation order of the wave-wide reductions and of the
// matrix products.  The polish is split the same way (polish_w); the start
// and the output are solve_quad's (start_stage_q, emit_q on quad 0).  The
// QP's workspace in LDS (LD = 1), stage data already staged (stage_in_q).
//
// Between the per-stage and the serial parts the values go through the
// workspace: pass 1's per-stage part leaves e in E, the gradients in GA and
// Sigma of the lane's components in DXA / DUA (dead until pass 2 writes the
// predictor); its first half leaves x_k (after the step) in E and the later
// stage's A'pi + H2xu u term in PV (both dead until the factorisation).
#pragma once

#include "ipm_quad.hpp"

namespace mpcqp {
namespace ipmw {

using namespace ipmq;

// sum over the whole wave (every lane ends with the total)
MPCQP_QD double wsum(double v) {
  v += lane_step<1>(v);
  v += lane_step<2>(v);
  v += lane_step<4>(v);
  v += lane_step<8>(v);
  v += lane_step<16>(v);
  v += lane_step<32>(v);
  return v;
}
MPCQP_QD double wave_max(double v) {
  v = fmax(v, lane_step<1>(v));
  v = fmax(v, lane_step<2>(v));
  v = fmax(v, lane_step<4>(v));
  v = fmax(v, lane_step<8>(v));
  v = fmax(v, lane_step<16>(v));
  return fmax(v, lane_step<32>(v));
}
MPCQP_QD double wave_min(double v) {
  v = fmin(v, lane_step<1>(v));
  v = fmin(v, lane_step<2>(v));
  v = fmin(v, lane_step<4>(v));
  v = fmin(v, lane_step<8>(v));
  v = fmin(v, lane_step<16>(v));
  return fmin(v, lane_step<32>(v));
}
MPCQP_QD double from_lane0(double v) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(bits & 0xffffffffll));
  const int hi = __builtin_amdgcn_readfirstlane((int)(bits >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
MPCQP_QD bool from_lane0(bool v) { return __builtin_amdgcn_readfirstlane(v ? 1 : 0) != 0; }

constexpr int kQuads = kWave / 4;

// ------------------------------------------------ Riccati on the matrix cores
// The factorisation sweep of riccati_q as 4 x 4 fp64 matrix products on
// v_mfma_f64_4x4x4_4b_f64 (measured on gfx950, tools/mfma64_probe): four
// independent 4 x 4 x 4 blocks, block m = (lane >> 2) & 3; in a block the B,
// C and D operands hold X[r][c] at lane 16 r + 4 m + c ("D layout") and the A
// operand reads a D-layout matrix as its transpose.  So with every stage
// matrix in D layout (lane (r, c) loads its element):
//   M1a = P'A = PA,  M1b = P [B | e] + [0 | p]        (2 products)
//   A'PA, A'M1b, B'PA, B'M1b                           (4 products)
//   K = -G^-1 Hx,  Ph = A'PA + Hx'K,  ph = A'Pe + Hx'k (3 products)
// with Hx = H2xu' + B'PA; the 2 x 2 block G, h is read from block 0 and
// inverted on every lane.  One stage is ~50 instructions with a dependency
// chain of 5 products, against ~285 VALU for the quad step (each fp64 VALU
// op issues in 4 cycles; a dependent 4x4x4 product returns in 23-29, a
// dependent FMA in 6.5: profiles/r06/mfma64_probe.txt).  All four blocks
// compute the same stage; block 0 stores.  Fields: the factor data as
// store_factor_q writes them (PP, KM, GI, KV, PV; E is not rewritten);
// the gradient g_x, the input gradients, Sigma_x and Sigma_u come from the
// lane-relative field FGX, the fields FGU, FGU+1, the lane-relative FSX and
// FSU, FSU+1.  Returns (uniformly) whether every G was positive definite.
MPCQP_QD double mfma44(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}
MPCQP_QD double lane_bcast(double v, int l) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffll), l);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int FGX, int FGU, int FSX, int FSU>
MPCQP_QD bool riccati_mfma(double* W, int N, double dreg) {
  const int lane = (int)threadIdx.x;
  const int r = lane >> 4, c = lane & 3;
  const bool store = ((lane >> 2) & 3) == 0;
  const bool isB = c < 2, isE = c == 2, isD = r == c, rowU = r < 2;
  // lane-constant offsets of the lane's element in a stage's fields
  const int oA = L::DA + r * NX + c;
  const int oB = L::DB + r * NU + (c & 1);
  const int oE = L::E + r;
  const int oWXX = L::WXX + pk(r, c);
  const int oSX = FSX + r, oGX = FGX + r;
  const int oWXU = L::WXU + c * NU + (r & 1);
  const int oPP = L::PP + pk(r, c), oKM = L::KM + (r & 1) * NX + c;
  // the stage's operands, loaded one stage ahead (the LDS round trip then
  // overlaps the previous stage's products instead of opening each stage)
  struct Ops {
    double a, bq, e, wxx, sx, gx, wxu, wuu0, wuu1, wuu2, su0, su1, gu0, gu1;
  };
  auto load = [&](int k) {
    const double* S = W + k * L::F;
    Ops o;
    o.a = S[oA]; o.bq = S[oB]; o.e = S[oE]; o.wxx = S[oWXX];
    o.sx = S[oSX]; o.gx = S[oGX]; o.wxu = S[oWXU];
    o.wuu0 = S[L::WUU]; o.wuu1 = S[L::WUU + 1]; o.wuu2 = S[L::WUU + 2];
    o.su0 = S[FSU]; o.su1 = S[FSU + 1]; o.gu0 = S[FGU]; o.gu1 = S[FGU + 1];
    return o;
  };
  double Ph = 0.0, phc = 0.0;
  bool ok = true;
  Ops nx = load(N - 1);
  for (int k = N - 1; k >= 0; --k) {
    double* S = W + k * L::F;
    const Ops o = nx;
    // P = Q' + H2xx + Ph + Sigma_x (+ shift), p = g_x + ph (column 2)
    const double P = o.wxx + Ph + (isD ? o.sx + dreg : 0.0);
    const double p = o.gx + phc;
    const double M1a = mfma44(P, o.a, 0.0);
    const double M1b = mfma44(P, isB ? o.bq : (isE ? o.e : 0.0), isE ? p : 0.0);
    // the next stage's operands, issued behind the first products (the
    // scheduler would otherwise sink them to their use: an LDS round trip
    // at the head of every stage)
    __builtin_amdgcn_sched_barrier(0);
    nx = load(k > 0 ? k - 1 : 0);
    __builtin_amdgcn_sched_barrier(0);
    const double Bz = isB ? o.bq : 0.0;
    const double AtPA = mfma44(o.a, M1a, 0.0);
    const double AtM1b = mfma44(o.a, M1b, 0.0);
    const double BtPA = mfma44(Bz, M1a, 0.0);
    const double BtM1b = mfma44(Bz, M1b, 0.0);
    // G = R + H2uu + Sigma_u + B'PB, h = g_u + B'Pe (block 0, lanes 0, 16, 17; 2, 18)
    double G[3], Gi[3];
    G[0] = o.wuu0 + o.su0 + dreg + lane_bcast(BtM1b, 0);
    G[1] = o.wuu1 + lane_bcast(BtM1b, 16);
    G[2] = o.wuu2 + o.su1 + dreg + lane_bcast(BtM1b, 17);
    const double h0 = o.gu0 + lane_bcast(BtM1b, 2), h1 = o.gu1 + lane_bcast(BtM1b, 18);
    ok = inv2(G, Gi) && ok;
    const double kk0 = -(Gi[0] * h0 + Gi[1] * h1), kk1 = -(Gi[1] * h0 + Gi[2] * h1);
    const double Hx = rowU ? BtPA + o.wxu : 0.0;
    const double mGi = (rowU && isB) ? -(r == c ? (r == 0 ? Gi[0] : Gi[2]) : Gi[1]) : 0.0;
    const double K = mfma44(mGi, Hx, 0.0);
    const double kkv = (rowU && isE) ? (r == 0 ? kk0 : kk1) : 0.0;
    Ph = mfma44(Hx, K, AtPA);
    phc = mfma44(Hx, kkv, AtM1b);
    if (store) {
      if (c <= r) S[oPP] = P;
      if (rowU) {
        S[oKM] = K;
        if (isE) S[L::KV + r] = kkv;
      }
      if (isE) S[L::PV + r] = p;
      if (r == 0 && c < 3) S[L::GI + c] = Gi[c];
    }
  }
  return ok;
}

// The two recursions that remain after the factorisation, on the matrix cores
// (same operand layouts as riccati_mfma; block 0 stores):
//  forward_mfma  dx_{k+1} = Acl_k dx_k + (e_k + B_k k_k), Acl = A + B K, the
//                state direction of x_{k+1} into the lane-relative field FOUT
//                (one dependent product per stage; the input direction
//                du_k = K_k dx_k + k_k is left to the per-stage phase after it,
//                du_of_stage);
//  rhs_mfma      the right-hand side sweep of rhs_sweep_q: p = g_x + phc,
//                Pe = P e + p, k = -G^-1 (g_u + B'Pe), phc = Acl'Pe + K'g_u
//                (one dependent product per stage).
// Acl' / Acl, P e + g_x and K'g_u do not depend on the recursion and are
// formed from the stage's fields ahead of it.
template <int FOUT>
MPCQP_QD void forward_mfma(double* W, int N) {
  const int lane = (int)threadIdx.x;
  const int r = lane >> 4, c = lane & 3;
  const bool store = ((lane >> 2) & 3) == 0 && c == 0, rowU = r < 2, col0 = c == 0;
  const int oKM = L::KM + (r & 1) * NX + c;
  const int oBt = L::DB + c * NU + (r & 1);
  const int oAt = L::DA + c * NX + r;
  const int oB0 = L::DB + r * NU, oE = L::E + r;
  // pipeline: the stage's raw operands two stages ahead, its closed-loop
  // matrix and offset (products that do not depend on the recursion) one
  // stage ahead, each behind a scheduling barrier after the recursion's
  // product of the current stage
  struct Raw {
    double Kd, Bt, At, b0, b1, e, kk0, kk1;
  };
  auto load = [&](int k) {
    const double* S = W + k * L::F;
    Raw o;
    o.Kd = rowU ? S[oKM] : 0.0; o.Bt = rowU ? S[oBt] : 0.0; o.At = S[oAt];
    o.b0 = S[oB0]; o.b1 = S[oB0 + 1]; o.e = S[oE];
    o.kk0 = S[L::KV]; o.kk1 = S[L::KV + 1];
    return o;
  };
  auto prep = [&](const Raw& o, double& AclT, double& ccl) {
    AclT = mfma44(o.Kd, o.Bt, o.At);  // (A + B K)'
    ccl = col0 ? fma(o.b1, o.kk1, fma(o.b0, o.kk0, o.e)) : 0.0;
  };
  double dx = 0.0;  // column 0: the direction of x_k
  double AclT, ccl;
  prep(load(0), AclT, ccl);
  Raw nx = load(N > 1 ? 1 : 0);
  for (int k = 0; k < N; ++k) {
    dx = mfma44(AclT, dx, ccl);
    __builtin_amdgcn_sched_barrier(0);
    prep(nx, AclT, ccl);
    nx = load(k + 2 < N ? k + 2 : N - 1);
    __builtin_amdgcn_sched_barrier(0);
    if (store) W[k * L::F + FOUT + r] = dx;
  }
}

template <int FGX, int FGU>
MPCQP_QD void rhs_mfma(double* W, int N) {
  const int lane = (int)threadIdx.x;
  const int r = lane >> 4, c = lane & 3;
  const bool store = ((lane >> 2) & 3) == 0 && c == 0, rowU = r < 2, col0 = c == 0;
  const int oPP = L::PP + pk(r, c), oE = L::E + r, oGX = FGX + r;
  const int oA = L::DA + r * NX + c, oKM = L::KM + (r & 1) * NX + c;
  const int oBt = L::DB + c * NU + (r & 1);
  // pipeline as forward_mfma: raw operands two stages ahead, the products
  // that do not depend on the recursion one stage ahead
  struct Raw {
    double P, e, gx, A, Kd, Bt, guc;
  };
  auto load = [&](int k) {
    const double* S = W + k * L::F;
    Raw o;
    o.P = S[oPP]; o.e = col0 ? S[oE] : 0.0; o.gx = col0 ? S[oGX] : 0.0;
    o.A = S[oA]; o.Kd = rowU ? S[oKM] : 0.0; o.Bt = rowU ? S[oBt] : 0.0;
    o.guc = (rowU && col0) ? S[FGU + (r & 1)] : 0.0;
    return o;
  };
  auto prep = [&](const Raw& o, double& Pe0, double& Acl, double& Ktgu, double& gx) {
    Pe0 = mfma44(o.P, o.e, o.gx);      // P e + g_x (column 0)
    Acl = mfma44(o.Bt, o.Kd, o.A);     // A + B K
    Ktgu = mfma44(o.Kd, o.guc, 0.0);   // K'g_u (column 0)
    gx = o.gx;
  };
  double phc = 0.0;  // column 0
  double Pe0, Acl, Ktgu, gx;
  prep(load(N - 1), Pe0, Acl, Ktgu, gx);
  Raw nx = load(N > 1 ? N - 2 : 0);
  for (int k = N - 1; k >= 0; --k) {
    const double p = gx + phc;
    phc = mfma44(Acl, Pe0 + phc, Ktgu);
    __builtin_amdgcn_sched_barrier(0);
    prep(nx, Pe0, Acl, Ktgu, gx);
    nx = load(k > 1 ? k - 2 : 0);
    __builtin_amdgcn_sched_barrier(0);
    if (store) W[k * L::F + L::PV + r] = p;
  }
}

// The feed-forward of stage k after rhs_mfma, lane i of a quad (lanes 0, 1
// store): k = -G^-1 (g_u + B'(P e + p)), g_u from FGU, FGU+1
template <int FGU>
MPCQP_QD void rhs_kk_stage(const WsQ<1>& at, int k, int i) {
  double Pe = at.r(k, L::PV);
#pragma unroll
  for (int j = 0; j < 4; ++j) Pe = fma(at.p(k, L::PP, j), at(k, L::E + j), Pe);
  double Pea[4];
  bcast4(Pe, Pea);
  double h[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double s = at(k, FGU + r);
#pragma unroll
    for (int q = 0; q < 4; ++q) s = fma(at(k, L::DB + q * NU + r), Pea[q], s);
    h[r] = s;
  }
  const double Gi[3] = {at(k, L::GI + 0), at(k, L::GI + 1), at(k, L::GI + 2)};
  if (i < 2) {
    const double kk = -(Gi[pk(i, 0)] * h[0] + Gi[pk(i, 1)] * h[1]);
    at.r(k, L::KV) = kk;
  }
}

// du_k = K_k dx_k + k_k of stage k, lane i < 2 (dx_k: the state direction of
// stage k-1 in the lane-relative field FDX, 0 at k = 0)
template <int FDX>
MPCQP_QD double du_of_stage(const WsQ<1>& at, int k, int i) {
  double s = at(k, L::KV + (i & 1));
  if (k > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s = fma(at(k, L::KM + (i & 1) * NX + j), at(k - 1, FDX + j), s);
  }
  return s;
}

// The backward sweep of a right-hand side on the stored factorisation (quad
// 0; the chain of pass 3, ipmq::rhs_step_q): g_x row i from field FGX
// (lane-relative), g_u (both inputs) from FGU; writes k -> KV and p -> PV
// (each stage's fields are read before they are written).
template <int FGX, int FGU>
MPCQP_QD void rhs_sweep_q(const WsQ<1>& at, int N, int i) {
  double phc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    const double gu[2] = {at(k, FGU), at(k, FGU + 1)};
    rhs_step_q(at, i, k, at.r(k, FGX), gu, phc);
  }
}

// ------------------------------------------------------- the serial chains
// The three recursions over the horizon, on the matrix cores or
// (-DMPCQP_RICCATI_QUAD, the A/B build) on quad 0 with ipm_quad.hpp's helpers.
// All 64 lanes call them; the caller synchronises the workspace before and
// after.  qd = the lane's quad, i = its lane in the quad.
//
// factor   the Riccati factorisation from e in E, g_x in FGX (lane-relative),
//          g_u in FGU, FGU+1, Sigma_x in FSX (lane-relative), Sigma_u in FSU,
//          FSU+1 -> PP, KM, GI, KV, PV; wave-uniform: every pivot positive.
template <int FGX, int FGU, int FSX, int FSU>
MPCQP_QD bool factor(const WsQ<1>& at, int N, int qd, int i, double dreg) {
#ifndef MPCQP_RICCATI_QUAD
  return riccati_mfma<FGX, FGU, FSX, FSU>(at.W, N, dreg);
#else
  bool pd = true;
  if (qd == 0) {
    double Ph[4] = {0.0, 0.0, 0.0, 0.0}, ph = 0.0;
    for (int k = N - 1; k >= 0; --k) {
      StageQ S;
      S.load(at, k);
      const double e = at.r(k, L::E), gx = at.r(k, FGX), sx = at.r(k, FSX);
      const double gu[2] = {at(k, FGU), at(k, FGU + 1)};
      const double su2[2] = {at(k, FSU), at(k, FSU + 1)};
      double P[4], p, K[2][4], kk[2], Gi[3], Kc[2];
      pd = riccati_q(at, S, k, i, Ph, ph, e, gx, gu, sx, su2, dreg, P, p, K, kk, Gi, Kc) && pd;
      store_factor_q(at, k, i, P, p, Kc, kk, Gi, e);
    }
  }
  return from_lane0(pd);
#endif
}

// rhs      a right-hand side on the stored factorisation: g_x in FGX, g_u in
//          FGU, FGU+1 -> p in PV, k in KV.
template <int FGX, int FGU>
MPCQP_QD void rhs(const WsQ<1>& at, int N, int qd, int i) {
#ifndef MPCQP_RICCATI_QUAD
  rhs_mfma<FGX, FGU>(at.W, N);
  wave_lds_sync();
  // (g_u may be in KV: every stage reads its own before writing k there)
  for (int k = qd; k < N; k += kQuads) rhs_kk_stage<FGU>(at, k, i);
#else
  if (qd == 0) rhs_sweep_q<FGX, FGU>(at, N, i);
#endif
}

// forward  the state direction of x_{k+1} -> the lane-relative field FDX of
//          stage k; the input direction of a stage is du_of_stage<FDX>.
template <int FDX>
MPCQP_QD void forward(const WsQ<1>& at, int N, int qd, int i) {
#ifndef MPCQP_RICCATI_QUAD
  forward_mfma<FDX>(at.W, N);
#else
  if (qd == 0)
    forward_q(at, N, i, [&](int k, const double (&)[2], double dxn, const double (&)[4]) {
      at.r(k, FDX) = dxn;
    });
#endif
}

// What stage k needs from the stage after it: A_{k+1}'pi_{k+2} + H2xu_{k+1}
// u_{k+1}, row i, from that stage's pi in FPI and u in FU, each plus alpha
// times FDPI / FDU when alpha > 0 (its step not yet applied); 0 at the last
// stage.
template <int FPI, int FU, int FDPI, int FDU>
MPCQP_QD double later_gx1(const WsQ<1>& at, int N, int i, int k, double alpha) {
  if (k + 1 >= N) return 0.0;
  const bool ou = i < NU;
  double pin = at.r(k + 1, FPI), un = ou ? at.r(k + 1, FU) : 0.0;
  if (alpha > 0.0) {
    pin += alpha * at.r(k + 1, FDPI);
    if (ou) un += alpha * at.r(k + 1, FDU);
  }
  double pia[4], ua[2];
  bcast4(pin, pia);
  ua[0] = qb<0>(un);
  ua[1] = qb<1>(un);
  StageQ S;
  return next_gx1_q(at, S, k + 1, i, pia, ua);
}

// polish_q (ipm_quad.hpp) on the whole wave: each method-of-multipliers step
// is the per-stage residual / gradient / penalty (one quad per
// stage, into the factor fields the serial sweep overwrites after reading: e
// -> E, g_x -> PV, g_u -> KV, the penalties -> KM / GI), the Riccati sweep
// (factor; rhs where the factors stand), the forward sweep (the state
// direction of stage k -> E), then per stage the step, the costate update, the
// multipliers and the active-set tests (polish_check_q).  Returns
// (wave-uniform) whether the polish certified its vertex.
template <typename T>
MPCQP_QD bool polish_w(const Args<T>& a, const WsQ<1>& at, int qd, int i, double x0i,
                       bool warm) {
  const int N = a.N;
  const bool ou = i < NU;
  for (int k = qd; k < N; k += kQuads) polish_init_q(at, i, k, warm);
  wave_lds_sync();
  const int rounds = polish_rounds(warm);
  for (int round = 0; round < rounds; ++round) {
    bool good = true, changed = false;
    for (int step = 0; step < kPolishSteps; ++step) {
      const double rho = polish_rho(step);
      // the last step keeps the penalty of the one before: same factorisation
      const bool refactor = step < 3;
      // per stage: residual, gradients and the active components' penalty
      // (polish_grad_q's statements on their own text: as that call, this
      // kernel measured 0.8 % slower)
      for (int k = qd; k < N; k += kQuads) {
        const double xi = at.r(k, L::DX), pii = at.r(k, L::DPI);
        const double ui = ou ? at.r(k, L::DU) : 0.0;
        const double xki = k == 0 ? x0i : at.r(k - 1, L::DX);
        double gx1 = 0.0;
        if (k + 1 < N) {
          const double pin = at.r(k + 1, L::DPI), un = ou ? at.r(k + 1, L::DU) : 0.0;
          double pia[4], ua[2];
          bcast4(pin, pia);
          ua[0] = qb<0>(un);
          ua[1] = qb<1>(un);
          StageQ S1;
          gx1 = next_gx1_q(at, S1, k + 1, i, pia, ua);
        }
        double xa[4], x1a[4], pia[4], ua[2];
        bcast4(xki, xa);
        bcast4(xi, x1a);
        bcast4(pii, pia);
        ua[0] = qb<0>(ui);
        ua[1] = qb<1>(ui);
        StageQ S;
        S.load(at, k);
        const double e = resid_q(at, S, k, i, xa, ua, xi);
        double gx, gu[2];
        grad_q(at, S, k, i, xa, x1a, pia, ua, pii, gx1, gx, gu);
        double sx = 0.0, sui = 0.0;
        {
          const int j = NU + i;
          const double act = at(k, L::GA + j);
          if (act != 0.0) {
            const double bnd = act > 0.0 ? at(k, L::HI + j) : at(k, L::LO + j);
            sx = rho;
            gx += at.r(k, L::DXA) + rho * (xi - bnd);
          }
        }
        double gum = 0.0;
        if (ou) {
          const double act = at.r(k, L::GA);
          if (act != 0.0) {
            const double bnd = act > 0.0 ? at.r(k, L::HI) : at.r(k, L::LO);
            sui = rho;
            gum = at.r(k, L::DUA) + rho * (ui - bnd);
          }
        }
        gu[0] += qb<0>(gum);
        gu[1] += qb<1>(gum);
        at.r(k, L::E) = e;
        at.r(k, L::PV) = gx;
        if (ou) at.r(k, L::KV) = sel2(gu, i);
        if (refactor) {  // (a kept factorisation keeps its K and G^-1 fields)
          at.r(k, L::KM) = sx;
          if (ou) at.r(k, L::GI) = sui;
        }
      }
      wave_lds_sync();
      // the penalty and the active set of the previous step: its factors
      // stand, only the right-hand side is swept
      if (refactor) good = factor<L::PV, L::KV, L::KM, L::GI>(at, N, qd, i, 0.0) && good;
      else rhs<L::PV, L::KV>(at, N, qd, i);
      wave_lds_sync();
      forward<L::E>(at, N, qd, i);
      wave_lds_sync();
      // the step: x, u += the directions (the state direction of stage k is
      // in E(k); du_k needs that of stage k-1, so the updates of DX follow)
      for (int k = qd; k < N; k += kQuads)
        if (ou) at.r(k, L::DU) += du_of_stage<L::E>(at, k, i);
      wave_lds_sync();
      for (int k = qd; k < N; k += kQuads) at.r(k, L::DX) += at.r(k, L::E);
      wave_lds_sync();
      const bool last = step == kPolishSteps - 1;
      const bool probe = !last && step >= kPolishEarly;
      bool pass = true;
      for (int k = qd; k < N; k += kQuads) {
        const double dxa[4] = {at(k, L::E + 0), at(k, L::E + 1), at(k, L::E + 2), at(k, L::E + 3)};
        polish_check_q(at, i, k, dxa, at.r(k, L::DX), ou ? at.r(k, L::DU) : 0.0, rho, last, probe,
                       good, changed, pass);
      }
      wave_lds_sync();
      if (probe && wave_min(good && pass ? 1.0 : 0.0) > 0.5) return true;
    }
    good = wave_min(good ? 1.0 : 0.0) > 0.5;
    changed = wave_max(changed ? 1.0 : 0.0) > 0.5;
    if (good && !changed) return true;
    if (!good) return false;
  }
  return false;
}

// All 64 lanes, uniform control flow; returns true (on every lane) when the
// QP ended polished.  warm, pclk: as solve_quad.
template <typename T>
MPCQP_QD bool solve_wave(const Args<T>& a, int b, double* W, bool warm = false,
                         uint64_t* pclk = nullptr) {
#ifdef MPCQP_IPM_PASSCLK
  uint64_t pclk_t = __builtin_amdgcn_s_memrealtime();
#endif
  const int lane = (int)threadIdx.x, qd = lane >> 2;
  const int i = lane & 3;
  const bool q0 = qd == 0;
  const WsQ<1> at(W, i);
  const bool ou = i < NU;
  const int N = a.N;
  const double x0i = i < a.nx ? (double)a.x0[(int64_t)b * a.sX0 + i] : 0.0;

  // ------------------------------------------------- start (quad 0, serial)
  double mc = 0.0;
  if (q0) {
    double xi = x0i;
    for (int k = 0; k < N; ++k) start_stage_q(a, b, at, i, k, xi, mc);
  }
  const double mcount = wsum(mc);
  wave_lds_sync();
  MPCQP_PCLK(6);
  if (warm && mcount > 0.0) {
    const bool wp = polish_w<T>(a, at, qd, i, x0i, true);
    MPCQP_PCLK(7);
    if (wp) {
      if (q0) emit_q<T>(a, b, at, i, true, MPCQP_STATUS_OPTIMAL, 0);
      return true;
    }
  }

  ipm::Control c;
  c.mu_pol = a.mu_polish;
  for (int it = 0;; ++it) {
    // ========================= pass 1a: per stage, the neighbours' values
    // x_k after the previous step (stage k-1's state, not yet updated in
    // solve_quad's backward order) -> E; the later stage's A'pi + H2xu u
    // after the step -> PV
    for (int k = qd; k < N; k += kQuads) {
      double xki = k == 0 ? x0i : at.r(k - 1, L::X);
      if (c.alpha > 0.0 && k > 0) xki += c.alpha * at.r(k - 1, L::DX);
      const double gx1 = later_gx1<L::PI, L::U, L::DPI, L::DU>(at, N, i, k, c.alpha);
      at.r(k, L::E) = xki;
      at.r(k, L::PV) = gx1;
    }
    wave_lds_sync();
    MPCQP_PCLK(8);
    // ============ pass 1b: per stage, the step, residual, gradients, Sigma
    double rstat = 0.0, rdyn = 0.0, musum = 0.0;
    for (int k = qd; k < N; k += kQuads) {
      StageOutQ o;
      pass1_stage_q(at, i, k, at.r(k, L::E), at.r(k, L::PV), c, rstat, rdyn, musum, o);
      if (ou) at.r(k, L::DUA) = o.sui;
      at.r(k, L::E) = o.e;
      at.r(k, L::DXA) = o.sx;
    }
    wave_lds_sync();
    MPCQP_PCLK(9);
    // ============================== pass 1c: the Riccati factorisation
    const bool pd = factor<L::GA + NU, L::GA, L::DXA, L::DUA>(at, N, qd, i, c.dreg);
    MPCQP_PCLK(10);
    rstat = wave_max(rstat);
    rdyn = wave_max(rdyn);
    const double mu = mcount > 0.0 ? wsum(musum) / mcount : 0.0;
    wave_lds_sync();
    ipm::Next next = ipm::after_factor(c, a, it, pd, rstat, rdyn, mu, mcount > 0.0);
    if (next == ipm::kPolish) {
      MPCQP_PCLK(0);
      const bool pol = polish_w<T>(a, at, qd, i, x0i, false);
      MPCQP_PCLK(4);
      if (pol) {
        if (q0) emit_q<T>(a, b, at, i, true, MPCQP_STATUS_OPTIMAL, it);
        return true;
      }
      next = ipm::after_failed_polish(c, a, it);
    } else if (next == ipm::kAgain) {
      MPCQP_PCLK(5);
    }
    if (next == ipm::kStop) {
      if (q0) emit_q<T>(a, b, at, i, false, c.code, it);
      return false;
    }
    if (next == ipm::kAgain) continue;

    MPCQP_PCLK(0);
    // ============ pass 2: the predictor's forward sweep, then per stage
    forward<L::DXA>(at, N, qd, i);
    wave_lds_sync();
    double amax = 1.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (int k = qd; k < N; k += kQuads) {
      const double dun = ou ? du_of_stage<L::DXA>(at, k, i) : 0.0;
      if (ou) at.r(k, L::DUA) = dun;
      pass2_stage_q(at, i, k, at.r(k, L::DXA), dun, amax, c0, c1, c2);
    }
    amax = wave_min(amax);
    c.sigmu = ipm::centering(mcount, wsum(c0), wsum(c1), wsum(c2), amax, mu);

    MPCQP_PCLK(1);
    // ==== pass 3: per stage the corrector right-hand side (-> GA), then the
    // backward chain
    for (int k = qd; k < N; k += kQuads) {
      double gx, gum;
      pass3_stage_q(at, i, k, c.sigmu, gx, gum);
      if (ou) at.r(k, L::GA) = gum;
      at.r(k, L::GA + NU) = gx;
    }
    wave_lds_sync();
    rhs<L::GA + NU, L::GA>(at, N, qd, i);
    wave_lds_sync();

    MPCQP_PCLK(2);
    // ========== pass 4: the corrector's forward sweep, then per stage
    forward<L::DX>(at, N, qd, i);
    wave_lds_sync();
    amax = 1.0;
    for (int k = qd; k < N; k += kQuads) {
      const double dun = ou ? du_of_stage<L::DX>(at, k, i) : 0.0;
      if (ou) at.r(k, L::DU) = dun;
      const double dxa[4] = {at(k, L::DX + 0), at(k, L::DX + 1), at(k, L::DX + 2), at(k, L::DX + 3)};
      pass4_stage_q(at, i, k, at.r(k, L::DX), dun, dxa, c.sigmu, amax);
    }
    c.alpha = ipm::step_length(wave_min(amax));
    wave_lds_sync();
    MPCQP_PCLK(3);
  }
}

}  // namespace ipmw
}  // namespace mpcqp
