// Body of the constitutive kernel entries of model_kernel.hpp (k_model_setup, k_model_setup_rec_nt), included INSIDE their function bodies: no header of its own.
// In scope: the template parameters KIN, LVEC, NFIX, QB, REC, STG, LEAN, the kernel arguments of k_model_setup and the launch policy TAIL, WJ.
   static_assert(TAIL || (QB && !STG && !ecmdev::kin_is_km(KIN)), "launch policy without tail split: the element-blocked per-lane Voce launches");
   // tail: list this launch works on (tail_mode) or appends to; tail_out: list a tail launch appends the points to that it cuts off itself
   // (second level); rs_in / rs_out: solver states of the listed points, [RS_N][P] by list slot (nullptr: a listed point starts over)
   if (!tail_out) tail_out = tail;
   // VG (p = 2, element-blocked): the geometry comes from the pre-pass (gen_kernels.hip, k_geom_p2) - Jio holds the Jacobians (input), `vel` the reference-space
   // velocity gradients dv_c/dxi_d, both (3,3,Q,E) - instead of 189 scattered loads per point.  With REC the launch writes the p = 2 record of the matrix-free
   // action (18 pairs: D, K, then adj(J) and W detJ - the latter five pairs right here in the prologue, where J is at hand).
   constexpr bool VG = !LVEC && NFIX == 27;
   static_assert(!VG || QB, "velocity-gradient input: element-blocked layout");
   // REC with STG (round 6): the fused p = 1 launch on the REFERENCE layout - state and stress rows staged, the record written per lane: for one pair the 8 points x
   // 8 consecutive elements of a wave store 8 whole 128-byte lines of the record array ([block][q][pair][lane = element])
   static_assert(!REC || (LVEC && NFIX == 8 && (QB || STG)) || (QB && VG), "record output: the fused p = 1 launches (element-blocked, or staged reference layout) and the p = 2 launch behind its geometry pre-pass");
   static_assert(!STG || (!QB && NFIX != 27), "staged rows: reference layout, generic or trilinear node loops");
   static_assert(!LEAN || (QB && REC), "lean end-of-step state: the element-blocked record launches");
   const int tail_mode = TAIL ? tail_mode_rt : 0;
   if (tail_mode && (int64_t)blockIdx.x * blockDim.x >= tail[0]) return;   // tail launch: its grid covers the worst case, blocks beyond the list leave before the table fill
   const int n = NFIX ? NFIX : n_rt;
   constexpr bool P2F = (NFIX == 27);   // triquadratic fused path: G holds the 3 x 6 one-dimensional tables, read through scalar loads
   // workgroups are dealt round-robin to the 8 XCDs.  (Remapped, so that an XCD works on one contiguous eighth of the element blocks and the node
   // gathers of neighbouring blocks hit the same L2, the launch ran 4.176 against 4.194 ms at 128^3: nothing, the kernel is issue-bound.)
   const int64_t bidx = blockIdx.x;
   // LDS: shape-derivative rows (not for P2F), the per-thread stash, the slip table (Kocks-Mecking).  A wave of the element-blocked launch works
   // on ONE point index q, so only the rows of the block's waves are staged (row w = the (n,3) table of wave w's q: 192 B per wave instead of
   // the 1.5 KB table - what lets four 128-thread blocks of the Kocks-Mecking kernels fit the 160 KB of a CU); the dense tail launch and the
   // reference layout have lane-varying q and stage the whole (n,3,Q) table (model_lds_bytes gives the launch the matching size)
   extern __shared__ double sG[];
   const bool rows_by_wave = QB && !tail_mode;
   const int wpb = (int)(blockDim.x >> 6);
   // fused trilinear launch, element-blocked: q is wave-uniform, so the 24 shape derivatives of the wave's point come through scalar loads
   // (no LDS staging, no barrier, no round trip in front of everything else); the dense tail launch (lane-varying q) stages the whole table
   constexpr bool SROW = LVEC && NFIX == 8 && QB;
   constexpr bool GSTG = STG && NFIX == 8;   // staged trilinear launch: every wave keeps its own copy of the 1.5 KB table in its stage while it forms L (no block barrier, no LDS beyond the stash)
   const bool g_lds = !P2F && !GSTG && !(SROW && rows_by_wave) && exa_g_in_lds(n, rows_by_wave ? wpb : Q);   // orders above 2: the table stays in global memory (exa_internal.hpp)
   const int tab = g_lds ? n * 3 * (rows_by_wave ? wpb : Q) : 0;
   // Kocks-Mecking: the slip table (12 rows of 8) behind the stash, for the rows that are read by lane-varying index (ecm_device.hpp, eval_rj)
   const int pqo = tab + EXA_STASH_DOUBLES;
   if (g_lds) for (int i = threadIdx.x; i < tab; i += blockDim.x) {
      const int row = i / (3 * n), k = i - row * (3 * n);
      sG[i] = G[3 * n * (rows_by_wave ? (int)((bidx * wpb + row) % Q) : row) + k];
   }
   if (ecmdev::kin_is_km(KIN)) for (int i = threadIdx.x; i < 8 * ecmdev::NSLIP; i += blockDim.x) sG[pqo + i] = (&ecmdev::PQ_TAB[0][0])[i];
   if (g_lds || ecmdev::kin_is_km(KIN)) __syncthreads();
   if (tail_mode) {   // dense pass over the points the capped launch handed over: thread t owns point tail[1 + t]
      const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= tail[0]) return;
      if (rs_in) rs_in += t;   // this point's slot
   }
   PointIO<QB, REC, STG, (NFIX == 27) ? PAC_PAIRS_GEO : PAC_PAIRS, TAIL> io{ state0, stress0, state1, stress1, cmat, sG + tab, tail, tail_mode, Q, bidx, wpb, 0, 0, 0, P, true };
   io.locate(threadIdx.x);
   const int q = io.q; const int64_t e = io.e;
   if (STG && !tail_mode) { if (io.nvalid() <= 0) return; }   // (wave-uniform: none of the wave's points exists)
   else if (!tail_mode && e * Q >= P) return;
   constexpr int QS = QB ? 64 : 1;
   // the point's begin-of-step state and stress are requested first: they depend on nothing but (e, q) and travel while the nodes are gathered
   ecmdev::PointIn pin;
   [[maybe_unused]] double2 rws[STG ? 14 : 1], rwt[STG ? 3 : 1];
   [[maybe_unused]] const int lane = (int)(threadIdx.x & 63);
   const double* Jq_in = nullptr; const double* ve_in = nullptr;   // !LVEC: this point's Jacobian row and its element's velocity E-vector row
   const bool staged = STG && !tail_mode;   // (kernel-uniform)
   if (STG && tail_mode) {   // dense launch of the staged kernel: scattered points, every input per lane (the 1.5 KB shape table from global memory: lanes
      // beyond the list have left, nothing here may need the whole wave; state and stress are requested behind the geometry - see below)
      if constexpr (!LVEC) { Jq_in = Jio + qview<QB>(9, Q, e, q).base; ve_in = vel + (int64_t)3 * n * e; }
   } else if constexpr (STG) {
      // (requested in the order of use - loads return in order: the geometry rows first, so that L is formed while the state rows are still on their way)
      const int nv = io.nvalid(); const int64_t p0 = io.pt0(); double* wr = io.wreg();
      [[maybe_unused]] double2 rg[2], rj[5], rv[2];
      if constexpr (GSTG) rows_load<2>(G, 192, lane, rg);
      if constexpr (!LVEC) {
         rows_load<5>(Jio + p0 * 9, nv * 9, lane, rj);
         if constexpr (NFIX == 8) rows_load<2>(vel + (p0 >> 3) * 24, (nv >> 3) * 24, lane, rv);   // Q = 8: the wave's 64 points are 8 whole elements, whose E-vector rows are contiguous
      }
      rows_load<14>(state0 + p0 * ecmdev::NSTATEV, nv * ecmdev::NSTATEV, lane, rws);
      rows_load<3>(stress0 + p0 * 6, nv * 6, lane, rwt);
      if constexpr (GSTG) rows_to_stage<2, 192>(wr + STG_G, lane, rg);
      if constexpr (!LVEC) {
         rows_to_stage<5, 576>(wr + STG_J, lane, rj);
         Jq_in = wr + STG_J + io.row_in() * 9;
         if constexpr (NFIX == 8) { rows_to_stage<2, 192>(wr + STG_V, lane, rv); ve_in = wr + STG_V + (io.row_in() >> 3) * 24; }
         else ve_in = vel + (int64_t)3 * n * e;
      }
      ECM_PARK_BARRIER(); __builtin_amdgcn_wave_barrier();
   } else {
      ecmdev::load_point_in<QS>(io.sv0(), io.s0(), pin);
      if constexpr (!LVEC) { Jq_in = Jio + qview<QB>(9, Q, e, q).base; ve_in = vel + (int64_t)3 * n * e; }
   }
   const QView vJ = qview<QB>(9, Q, e, q);
   const double* Gq = (GSTG && staged) ? io.wreg() + STG_G + 24 * q : (g_lds ? sG + 3 * n * (rows_by_wave ? (int)(threadIdx.x >> 6) : q) : G + 3 * n * q);
   // Jacobian output of an LVEC launch: the point's slot, or (STG) its row of the stage, stored by the wave once all 64 rows are there
   auto store_J = [&](const double a11, const double a21, const double a31, const double a12, const double a22, const double a32, const double a13, const double a23, const double a33) {
      if (STG && staged) {
         double* Jo = io.wreg() + STG_J + (int)(threadIdx.x & 63) * 9;
         Jo[0] = a11; Jo[1] = a21; Jo[2] = a31; Jo[3] = a12; Jo[4] = a22; Jo[5] = a32; Jo[6] = a13; Jo[7] = a23; Jo[8] = a33;
         ECM_PARK_BARRIER(); __builtin_amdgcn_wave_barrier();
         io.template flush_rows<9, 9>(io.wreg() + STG_J, Jio + io.pt0() * 9, io.nvalid() * 9);
      } else {
         double* Jo = Jio + vJ.base;
         ecmdev::stg(Jo, a11); ecmdev::stg(Jo + QS, a21); ecmdev::stg(Jo + 2 * QS, a31); ecmdev::stg(Jo + 3 * QS, a12); ecmdev::stg(Jo + 4 * QS, a22); ecmdev::stg(Jo + 5 * QS, a32);
         ecmdev::stg(Jo + 6 * QS, a13); ecmdev::stg(Jo + 7 * QS, a23); ecmdev::stg(Jo + 8 * QS, a33);
      }
   };
   double J11, J21, J31, J12, J22, J32, J13, J23, J33;
   double tsc = 0.0;   // REC: dt W_q / detJ
   double L[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
   if constexpr (VG) {
      const double* Jq = Jio + vJ.base; const double* Lq = vel + vJ.base;
      J11 = ecmdev::ldg(Jq); J21 = ecmdev::ldg(Jq + QS); J31 = ecmdev::ldg(Jq + 2 * QS); J12 = ecmdev::ldg(Jq + 3 * QS); J22 = ecmdev::ldg(Jq + 4 * QS); J32 = ecmdev::ldg(Jq + 5 * QS);
      J13 = ecmdev::ldg(Jq + 6 * QS); J23 = ecmdev::ldg(Jq + 7 * QS); J33 = ecmdev::ldg(Jq + 8 * QS);
      double gv[9];   // gv[c + 3 d] = dv_c/dxi_d
#pragma unroll
      for (int i = 0; i < 9; i++) gv[i] = ecmdev::ldg(Lq + i * QS);
      // adj(J) exactly as AssembleGradPA stores it (pa_kernels.hip, adj_det)
      const double a0 = J22 * J33 - J23 * J32, a1 = J32 * J13 - J12 * J33, a2 = J12 * J23 - J22 * J13;
      const double a3 = J31 * J23 - J21 * J33, a4 = J11 * J33 - J13 * J31, a5 = J21 * J13 - J11 * J23;
      const double a6 = J21 * J32 - J31 * J22, a7 = J31 * J12 - J11 * J32, a8 = J11 * J22 - J12 * J21;
      const double detJ = J11 * (J22 * J33 - J32 * J23) - J21 * (J12 * J33 - J32 * J13) + J31 * (J12 * J23 - J22 * J13);
      const double di = 1.0 / detJ;
      if constexpr (REC) {
         const int qu = tail_mode ? q : __builtin_amdgcn_readfirstlane(q);
         const double wq = tail_mode ? Wq[q] : p2::as_const(Wq)[qu];
         tsc = dt * wq * di;
         double2* rc = reinterpret_cast<double2*>(io.cm());
         ecmdev::stg2(&rc[13 * 64], a0, a1); ecmdev::stg2(&rc[14 * 64], a2, a3); ecmdev::stg2(&rc[15 * 64], a4, a5); ecmdev::stg2(&rc[16 * 64], a6, a7);
         ecmdev::stg2(&rc[17 * 64], a8, wq * (J11 * a0 + J21 * a1 + J31 * a2));      // W detJ with detJ as adj_det forms it
      }
      const double Ji[3][3] = { { di * (J22 * J33 - J23 * J32), di * (J32 * J13 - J12 * J33), di * (J12 * J23 - J22 * J13) },
                                { di * (J31 * J23 - J21 * J33), di * (J11 * J33 - J13 * J31), di * (J21 * J13 - J11 * J23) },
                                { di * (J21 * J32 - J31 * J22), di * (J31 * J12 - J11 * J32), di * (J11 * J22 - J12 * J21) } };
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int t = 0; t < 3; t++) L[c + 3 * t] = gv[c] * Ji[0][t] + gv[c + 3] * Ji[1][t] + gv[c + 6] * Ji[2][t];
   } else if constexpr (P2F) {
      static_assert(!P2F || LVEC, "the triquadratic fused path gathers from L-vectors");
      // both node contractions as three one-dimensional passes (p2_basis.hpp); q is wave-uniform except in the tail launch
      const int qu = (QB && !tail_mode) ? __builtin_amdgcn_readfirstlane(q) : q;
      p2::Rows r; p2::load_rows(p2::as_const(G), qu, r);
      const int32_t* ce = conn + (int64_t)27 * e;
      int gn[27];
#pragma unroll
      for (int a = 0; a < 27; a++) gn[a] = ce[a];
      double gx[3][3];
      p2::gather(r, [&](int a, int c) { return xl[gn[a] + (int64_t)nnodes * c]; }, gx);
      J11 = gx[0][0]; J21 = gx[1][0]; J31 = gx[2][0]; J12 = gx[0][1]; J22 = gx[1][1]; J32 = gx[2][1]; J13 = gx[0][2]; J23 = gx[1][2]; J33 = gx[2][2];
      store_J(J11, J21, J31, J12, J22, J32, J13, J23, J33);
      const double detJ = J11 * (J22 * J33 - J32 * J23) - J21 * (J12 * J33 - J32 * J13) + J31 * (J12 * J23 - J22 * J13);
      const double di = 1.0 / detJ;
      const double Ji[3][3] = { { di * (J22 * J33 - J23 * J32), di * (J32 * J13 - J12 * J33), di * (J12 * J23 - J22 * J13) },
                                { di * (J31 * J23 - J21 * J33), di * (J11 * J33 - J13 * J31), di * (J21 * J13 - J11 * J23) },
                                { di * (J21 * J32 - J31 * J22), di * (J31 * J12 - J11 * J32), di * (J11 * J22 - J12 * J21) } };
      p2::gather(r, [&](int a, int c) { return vel[gn[a] + (int64_t)nnodes * c]; }, gx);   // dv_c / dxi_s
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int t = 0; t < 3; t++) L[c + 3 * t] = gx[c][0] * Ji[0][t] + gx[c][1] * Ji[1][t] + gx[c][2] * Ji[2][t];
   } else if constexpr (LVEC && NFIX == 8) {
      // Trilinear fused launch: connectivity once, then the 24 coordinates AND the 24 velocities of the element in one round trip, then the
      // arithmetic.  (Written as two node loops - Jacobian, velocity gradient - the compiler re-read the connectivity for the second one and
      // issued the velocity gathers behind the Jacobian stores: five dependent memory round trips before the first state value was used.)
      const int32_t* ce = conn + (int64_t)8 * e;
      int gi[8];
#pragma unroll
      for (int r = 0; r < 8; r++) gi[r] = ce[r];
      double xs[3][8], vs[3][8];
#pragma unroll
      for (int r = 0; r < 8; r++) {
         xs[0][r] = xl[gi[r]]; xs[1][r] = xl[gi[r] + nnodes]; xs[2][r] = xl[gi[r] + 2 * (int64_t)nnodes];
         vs[0][r] = vel[gi[r]]; vs[1][r] = vel[gi[r] + nnodes]; vs[2][r] = vel[gi[r] + 2 * (int64_t)nnodes];
      }
      double Jc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, Lx[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };   // Jc[i + 3 j] = dx_i/dxi_j, Lx[c + 3 s] = dv_c/dxi_s
      double wq = 0.0;
      auto contract = [&](auto&& Gv) {
#pragma unroll
         for (int r = 0; r < 8; r++) {
            const double g0 = Gv(r), g1 = Gv(r + 8), g2 = Gv(r + 16);
#pragma unroll
            for (int c = 0; c < 3; c++) {
               Jc[c] += xs[c][r] * g0; Jc[c + 3] += xs[c][r] * g1; Jc[c + 6] += xs[c][r] * g2;
               Lx[c] += vs[c][r] * g0; Lx[c + 3] += vs[c][r] * g1; Lx[c + 6] += vs[c][r] * g2;
            }
         }
      };
      if (SROW && rows_by_wave) {
         const int qu = __builtin_amdgcn_readfirstlane(q);
         const p2::cptr Gc = p2::as_const(G) + 24 * qu;
         if (REC) wq = p2::as_const(Wq)[qu];
         contract([&](int i) { return Gc[i]; });
      } else {
         if (REC) wq = Wq[q];
         contract([&](int i) { return Gq[i]; });
      }
      J11 = Jc[0]; J21 = Jc[1]; J31 = Jc[2]; J12 = Jc[3]; J22 = Jc[4]; J32 = Jc[5]; J13 = Jc[6]; J23 = Jc[7]; J33 = Jc[8];
      if (WJ < 0 ? Jio != nullptr : WJ != 0) {   // optional (uniform): the driver's p = 1 record route needs no Jacobian field - its integrator kernels take the geometry from the nodes
         store_J(J11, J21, J31, J12, J22, J32, J13, J23, J33);
      }
      const double detJ = J11 * (J22 * J33 - J32 * J23) - J21 * (J12 * J33 - J32 * J13) + J31 * (J12 * J23 - J22 * J13);
      const double di = 1.0 / detJ;
      if (REC) tsc = dt * wq * di;
      const double Ji[3][3] = { { di * (J22 * J33 - J23 * J32), di * (J32 * J13 - J12 * J33), di * (J12 * J23 - J22 * J13) },
                                { di * (J31 * J23 - J21 * J33), di * (J11 * J33 - J13 * J31), di * (J21 * J13 - J11 * J23) },
                                { di * (J21 * J32 - J31 * J22), di * (J31 * J12 - J11 * J32), di * (J11 * J22 - J12 * J21) } };
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
         for (int tt = 0; tt < 3; tt++) L[c + 3 * tt] = Lx[c] * Ji[0][tt] + Lx[c + 3] * Ji[1][tt] + Lx[c + 6] * Ji[2][tt];
   } else {
   if (LVEC) {
      // J(i,j) = sum_r x_r,i dN_r/dxi_j   (column-major 3x3 per point, like MFEM's geometric factors after the re-layout)
      J11 = J21 = J31 = J12 = J22 = J32 = J13 = J23 = J33 = 0.0;
      const int32_t* ce = conn + (int64_t)n * e;
#pragma unroll
      for (int r = 0; r < n; r++) {
         const int g = ce[r];
         const double x0 = xl[g], x1 = xl[g + nnodes], x2 = xl[g + 2 * (int64_t)nnodes];
         const double g0 = Gq[r], g1 = Gq[r + n], g2 = Gq[r + 2 * n];
         J11 += x0 * g0; J21 += x1 * g0; J31 += x2 * g0;
         J12 += x0 * g1; J22 += x1 * g1; J32 += x2 * g1;
         J13 += x0 * g2; J23 += x1 * g2; J33 += x2 * g2;
      }
      if (WJ < 0 ? Jio != nullptr : WJ != 0) {   // optional (uniform): the driver's p = 1 record route needs no Jacobian field - its integrator kernels take the geometry from the nodes
         store_J(J11, J21, J31, J12, J22, J32, J13, J23, J33);
      }
   } else {
      const double* Jq = Jq_in;
      J11 = Jq[0]; J21 = Jq[QS]; J31 = Jq[2 * QS]; J12 = Jq[3 * QS]; J22 = Jq[4 * QS]; J32 = Jq[5 * QS]; J13 = Jq[6 * QS]; J23 = Jq[7 * QS]; J33 = Jq[8 * QS];
   }
   // inverse Jacobian (reference src/mechanics_kernels.cpp:38-61)
   const double detJ = J11 * (J22 * J33 - J32 * J23) - J21 * (J12 * J33 - J32 * J13) + J31 * (J12 * J23 - J22 * J13);
   const double di = 1.0 / detJ;
   if (REC) tsc = dt * Wq[q] * di;
   // Ji[s][t] = dxi_s/dx_t
   const double Ji[3][3] = { { di * (J22 * J33 - J23 * J32), di * (J32 * J13 - J12 * J33), di * (J12 * J23 - J22 * J13) },
                             { di * (J31 * J23 - J21 * J33), di * (J11 * J33 - J13 * J31), di * (J21 * J13 - J11 * J23) },
                             { di * (J21 * J32 - J31 * J22), di * (J31 * J12 - J11 * J32), di * (J11 * J22 - J12 * J21) } };
   // velocity gradient L(c,t) = sum_r v(r,c) dN_r/dx_t = (sum_r v(r,c) dN_r/dxi_s) dxi_s/dx_t: the reference-space gradient first
   // (9 multiply-adds per node), then one 3 x 3 product - instead of pushing every node's shape gradient through J^-1 (18 per node)
   const double* ve = ve_in;
   const int32_t* ce = conn + (int64_t)n * e;
   double Lx[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };   // Lx[c + 3 s] = d v_c / d xi_s
#pragma unroll
   for (int r = 0; r < n; r++) {
      const double g0 = Gq[r], g1 = Gq[r + n], g2 = Gq[r + 2 * n];
      double v0, v1, v2;
      if (LVEC) { const int g = ce[r]; v0 = vel[g]; v1 = vel[g + nnodes]; v2 = vel[g + 2 * (int64_t)nnodes]; }
      else { v0 = ve[r]; v1 = ve[r + n]; v2 = ve[r + 2 * n]; }
      Lx[0] += v0 * g0; Lx[1] += v1 * g0; Lx[2] += v2 * g0;
      Lx[3] += v0 * g1; Lx[4] += v1 * g1; Lx[5] += v2 * g1;
      Lx[6] += v0 * g2; Lx[7] += v1 * g2; Lx[8] += v2 * g2;
   }
#pragma unroll
   for (int c = 0; c < 3; c++)
#pragma unroll
      for (int tt = 0; tt < 3; tt++) L[c + 3 * tt] = Lx[c] * Ji[0][tt] + Lx[c + 3] * Ji[1][tt] + Lx[c + 6] * Ji[2][tt];
   }
   if constexpr (STG) { if (staged) {   // geometry done (J, velocity and table rows are in registers): the state and stress rows go through the stage
      ECM_PARK_BARRIER(); __builtin_amdgcn_wave_barrier();
      double* wr = io.wreg();
      rows_to_stage<14, 64 * ecmdev::NSTATEV, ecmdev::NSTATEV, RS_SV>(wr, lane, rws);
      rows_to_stage<3, 64 * 6, 6, RS_S>(wr + 64 * RS_SV, lane, rwt);
      ECM_PARK_BARRIER(); __builtin_amdgcn_wave_barrier();
      ecmdev::load_point_in<1, true>(wr + io.row_in() * RS_SV, wr + 64 * RS_SV + io.row_in() * RS_S, pin);
      ECM_PARK_BARRIER(); __builtin_amdgcn_wave_barrier();   // (the stash slots of point_update overwrite the rows)
   } else ecmdev::load_point_in<1>(io.sv0(), io.s0(), pin); }   // (dense launch: not across the gathers - their registers are what the staged form's row pieces need)
   // per-thread stash behind the shape table in LDS (PointIO::stash)
   // (STG: a lane beyond the last point repeats the last point to the end - it is neither listed nor counted)
   const bool mine = !STG || io.live;
   int rc;
   if constexpr (TAIL) rc = point_update<KIN, QS, REC, STG, LEAN>(mp, dt, L, io, mine ? kcap : (1 << 30), pin, sG + pqo, tsc, trd != 0,
                                                  TailIO{ tail_out, rs_out, tail_mode ? rs_in : nullptr, P, !tail_mode && rs_out != nullptr && mine });
   else rc = point_update<KIN, QS, REC, STG, LEAN, false>(mp, dt, L, io, 1 << 30, pin, sG + pqo, tsc, trd != 0);
   if (rc == 1 && mine) atomicAdd(fail, 1);
