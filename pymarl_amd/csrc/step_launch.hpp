// One QMIX / VDN / IQL train step's launches (the sequence mq_learner.hip's first comment maps), phase by phase, with
// the phase timer and the dispatch helpers that name a kernel template's instantiations once.
#pragma once
#include <cstdio>
#include <string>
#include <type_traits>

#include "gru_kernels.hpp"
#include "td_lambda_kernel.hpp"
#include "per_kernels.hpp"
#include "epymarl_kernels.hpp"
#include "hyper2_kernels.hpp"
#include "learner_handle.hpp"
#include "reduce_plan.hpp"

namespace {

struct PhaseTimer {
  mq_handle* h;
  hipStream_t s;
  int cur = -1;
  int idx(int p) const { return (int)(h->tstep % h->slots) * PH_N + p; }
  void begin(int p) {
    end();
    if (h->slots <= 0 || !((h->mask >> p) & 1u)) return;
    (void)hipEventRecord(h->ev0[idx(p)], s);
    h->ev_used[idx(p)] = 1;
    cur = p;
  }
  void end() {
    if (cur < 0) return;
    (void)hipEventRecord(h->ev1[idx(cur)], s);
    cur = -1;
  }
};

// The tile kernels' <KQ1> instantiations (gru_tiles.hpp tile_kq1), named once: f(std::integral_constant<int, KQ1>).
template <class F>
void dispatch_kq1(int kq1, F&& f) {
  if (kq1 == 8) f(std::integral_constant<int, 8>{});
  else if (kq1 == 20) f(std::integral_constant<int, 20>{});
  else if (kq1 == 40) f(std::integral_constant<int, 40>{});
  else if (kq1 == 72) f(std::integral_constant<int, 72>{});
  else f(std::integral_constant<int, 80>{});
}

// The unfused recurrence's <RW> instantiations (rows per workgroup), named once: 1, 2, 4 and, for MAX = 8 (the
// forward), 8.
template <int MAX, class F>
void dispatch_rw(int rw, F&& f) {
  if (rw == 1) f(std::integral_constant<int, 1>{});
  else if (rw == 2) f(std::integral_constant<int, 2>{});
  else if constexpr (MAX == 4) f(std::integral_constant<int, 4>{});
  else if (rw == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// One train step's launches, phase by phase in stream order. Which kernels run is plan_step's answer `p`
// (step_plan.hpp), fixed before the first launch; nothing here decides.
struct Step {
  mq_handle* h;
  const Dims d;
  const Rep rp;
  const Lay L;
  Work w;
  int32_t* curmax;
  hipStream_t s;
  PhaseTimer pt;
  const bool rnorm = false;   // reward standardisation is set (mq_set_reward_norm)
  const int64_t RT = (int64_t)d.Tp * d.R;
  int n_norm_part = 0;   // reduce(): the norm partials it left for mq_apply

  int forward(const StepPlan& p);
  int hypernet(const StepPlan& p);
  int mixer_tail(const StepPlan& p);
  int hypernet2_backward(const StepPlan& p);
  int bptt(const StepPlan& p);
  int reduce(const StepPlan& p);

  // The mixer tail's kernel for plan p.mix (MQ_MIX_*) with the flag set FULL (mix_kernels.hpp: the pass, MIX_PER,
  // MIX_RS) and the trailing arguments x that FULL asks for, in the order that header documents.
  template <int FULL, typename... X>
  void mix(const StepPlan& p, X... x) {
    const dim3 grid(p.nblk_mix), block(256);
    const float *P0 = h->on, *P1 = h->tg;
    if (p.mix == MQ_MIX_FAST16)
      hipLaunchKernelGGL((mix_fast_kernel<16, 16, FULL, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax, x...);
    else if (p.mix == MQ_MIX_FAST32)
      hipLaunchKernelGGL((mix_fast_kernel<32, 16, FULL, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax, x...);
    else if (p.mix == MQ_MIX_STREAM)
      hipLaunchKernelGGL((mix_kernel<true, FULL, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax, x...);
    else
      hipLaunchKernelGGL((mix_kernel<false, FULL, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax, x...);
  }
};

int Step::forward(const StepPlan& p) {
  const float *P0 = h->on, *P1 = h->tg;
  if (p.ffn) {
    // the feed-forward agent: three row-parallel GEMMs, both nets each (ffn_kernels.hpp)
    pt.begin(PH_FC1);
    {
      Fc1Prob p1{d, rp, h->on, h->tg, h->off[MQ_P_FC1_W], h->off[MQ_P_FC1_B], w.X1, w.XIN, RT};
      MQ_HIP(launch_gemm(p1, (int)RT, 2 * mq::H, 1, s));
    }
    pt.begin(PH_GRUF);
    {
      FfnHidProb ph{w.X1, h->on, h->tg, h->off[MQ_P_FFN_W], h->off[MQ_P_FFN_B], w.Hs, RT};
      MQ_HIP(launch_gemm(ph, (int)RT, mq::H, 2, s));
    }
    pt.begin(PH_FC2);
    {
      Fc2Prob p2{w.Hs, h->on, h->tg, h->off[MQ_P_FC2_W], h->off[MQ_P_FC2_B], w.Q, RT, d.A};
      MQ_HIP(launch_gemm(p2, (int)RT, d.A, 2, s));
    }
    return MQ_OK;
  }
  if (p.fwd == FWD_TILES) {
    // row tiles of 32 (two M-tiles) per workgroup, both nets: the recurrence and fc1 / W_ih / fc2 on MFMA
    pt.begin(PH_GRUF);
    const dim3 grid(16 * (((d.R + TR_F - 1) / TR_F + 7) / 8));   // row tiles x 2 nets, XCD-paired (gru_tiles.hpp)
    dispatch_kq1(p.kq1, [&](auto K) {
      hipLaunchKernelGGL(gru_fwd_tile_kernel<decltype(K)::value>, grid, dim3(512), 0, s, d, rp, P0, P1, L, w);
    });
    MQ_HIP(hipGetLastError());
  } else if (p.fwd != FWD_UNFUSED) {
    // one row per workgroup: fc1 / W_ih / fc2 ride on the recurrence's idle matrix cores (gru_fwd_fused.hpp)
    pt.begin(PH_GRUF);
    if (p.hyp_place == HYP_FWD_GRID) {
      launch_fwd_fused_hyp(s, d, rp, P0, P1, L, w);
    } else if (p.fwd == FWD_PAIR) {
      std::string stamp_path;   // diagnostic (MQ_DIAG pair_stamp=<file>): step stamps of the first 8 workgroups
      const bool want_stamp = env_item("MQ_DIAG", "pair_stamp", &stamp_path) && !stamp_path.empty();
      const int hsched = env_int("MQ_DIAG", "hyp_sched", kHypSched, 16);   // tuning: the in-loop tile schedule
      const int pair_hyp = p.hyp_place == HYP_PAIR_WAVES ? 2 : p.hyp_place == HYP_PAIR_EPI ? 1 : 0;
      // the stamp build has the 5-slot gather only: shapes past it run unstamped (never a partial gather)
      const bool stamp = want_stamp && d.Tp <= 512 && FCH * d.O <= 256 * 5;
      launch_fwd_pair(s, d, rp, P0, P1, L, w, pair_hyp, stamp, hsched);
      if (stamp) {
        std::vector<uint32_t> st((size_t)8 * PST);
        MQ_HIP(hipMemcpyAsync(st.data(), w.slab_rnn, st.size() * 4, hipMemcpyDeviceToHost, s));
        MQ_HIP(hipStreamSynchronize(s));
        if (FILE* f = fopen(stamp_path.c_str(), "ab")) { fwrite(st.data(), 4, st.size(), f); fclose(f); }
      }
    } else {
      launch_fwd_fused(dim3(d.R, 2), s, d, rp, P0, P1, L, w);
    }
    MQ_HIP(hipGetLastError());
  } else {
    pt.begin(PH_FC1);
    {
      // the dense agent-input copy (XIN) is dW1's operand, fused or not
      Fc1Prob p{d, rp, h->on, h->tg, h->off[MQ_P_FC1_W], h->off[MQ_P_FC1_B], w.X1, w.XIN, RT};
      MQ_HIP(launch_gemm(p, (int)RT, 2 * mq::H, 1, s));
    }
    pt.begin(PH_GI);
    {
      GiProb p{w.X1, h->on, h->tg, h->off[MQ_P_RNN_W_IH], h->off[MQ_P_RNN_B_IH], w.GI, RT};
      MQ_HIP(launch_gemm(p, (int)RT, mq::G3, 2, s));
    }
    pt.begin(PH_GRUF);
    dispatch_rw<8>(p.rw_fwd, [&](auto K) {
      constexpr int RW = decltype(K)::value;
      hipLaunchKernelGGL(gru_fwd_kernel<RW>, dim3((d.R + RW - 1) / RW, 2), dim3(256), 0, s, d, P0, P1, L, w);
    });
    MQ_HIP(hipGetLastError());
    pt.begin(PH_FC2);
    {
      Fc2Prob p{w.Hs, h->on, h->tg, h->off[MQ_P_FC2_W], h->off[MQ_P_FC2_B], w.Q, RT, d.A};
      MQ_HIP(launch_gemm(p, (int)RT, d.A, 2, s));
    }
  }
  return MQ_OK;
}

// The QMIX hypernet as a launch of its own (no forward carried it).
int Step::hypernet(const StepPlan& p) {
  if (p.hyp_place != HYP_OWN_LAUNCH) return MQ_OK;
  pt.begin(PH_HYP);
  if (p.hyper2) {
    // layer 1 (pre-activations A1, and S0), then layer 2 into HYP: both nets each (hyper2_kernels.hpp)
    const Hyp2Lay& y = h->y2;
    Hyp1Prob p1{d, rp, y, h->on, h->tg, h->A1, w.S0};
    MQ_HIP(launch_gemm(p1, d.M, y.N1, 2, s));
    Hyp2FwdProb p2{y, h->on, h->tg, h->A1, w.HYP, d.M, d.NH};
    MQ_HIP(launch_gemm(p2, d.M, d.NH, 2, s));
    return MQ_OK;
  }
  if (p.hyper == MQ_HYP_WS) {
    // wave-specialised weight streaming (hyper_kernel.hpp)
    MQ_LDS(hyper_ws_kernel<0>, hyper_ws_lds_bytes(d.S));
    hipLaunchKernelGGL(hyper_ws_kernel<0>, dim3((d.M + HYR - 1) / HYR, 2), dim3(HYWS_THREADS),
                       hyper_ws_lds_bytes(d.S), s, d, rp, (const float*)h->on, (const float*)h->tg, L, w.HYP,
                       w.S0);
    MQ_HIP(hipGetLastError());
  } else if (p.hyper == MQ_HYP_LDS) {
    const size_t dyn = HyperGeom(d.S, d.NH).lds_bytes();
    MQ_LDS(hyper_kernel<0>, dyn);
    hipLaunchKernelGGL(hyper_kernel<0>, dim3((d.M + HYR - 1) / HYR, 2), dim3(256), dyn, s, d, rp,
                       (const float*)h->on, (const float*)h->tg, L, w.HYP, w.S0);
    MQ_HIP(hipGetLastError());
  } else {
    HypProb p{d, rp, L, h->on, h->tg, w.HYP, w.S0};
    MQ_HIP(launch_gemm(p, d.M, d.NH, 2, s));
  }
  return MQ_OK;
}

int Step::mixer_tail(const StepPlan& p) {
  const mq_config& c = h->cfg;
  // the tail's trailing arguments (mix_kernels.hpp): the standardised rewards, y' out and the lambda targets in, the
  // PER weights in and the |td m| record out
  const float* const RS = h->RS;
  float* const YT = h->YT;
  const float* const G = h->G;
  const float* const W = h->per.weights;
  float* const TDA = h->TDA;
  pt.begin(PH_MIX);
  if (rnorm) {   // the batch's rewards into the running statistics, and RS: the rewards every launch below reads
    hipLaunchKernelGGL(reward_norm_kernel, dim3(1), dim3(RN_THREADS), 0, s, d, rp, h->rew_state, h->RS.p);
    MQ_HIP(hipGetLastError());
  }
  if (!p.lambda) {
    if (rnorm && p.per) mix<MIX_ONE_STEP | MIX_PER | MIX_RS>(p, RS, W, TDA);
    else if (rnorm) mix<MIX_ONE_STEP | MIX_RS>(p, RS);
    else if (p.per) mix<MIX_ONE_STEP | MIX_PER>(p, W, TDA);
    else mix<MIX_ONE_STEP>(p);
    MQ_HIP(hipGetLastError());
  } else {
    // TD(lambda): y' of every (t, b), the backward scan over t per episode, then the loss against its targets
    const int k = c.mixer == MQ_MIXER_NONE ? d.n : 1;
    const size_t dyn = td_lambda_lds_bytes(d.T, k);
    MQ_LDS(td_lambda_kernel, dyn);
    mix<MIX_LAMBDA_TARGETS>(p, YT, G);
    MQ_HIP(hipGetLastError());
    const float lg = (float)((double)c.td_lambda * (double)c.gamma);
    const float og = (float)((1.0 - (double)c.td_lambda) * (double)c.gamma);
    if (rnorm) {
      MQ_LDS(td_lambda_rs_kernel, dyn);
      hipLaunchKernelGGL(td_lambda_rs_kernel, dim3(d.B), dim3(256), dyn, s, d, rp, (const float*)YT, h->G, k, lg, og,
                         RS);
    } else {
      hipLaunchKernelGGL(td_lambda_kernel, dim3(d.B), dim3(256), dyn, s, d, rp, (const float*)YT, h->G, k, lg, og);
    }
    MQ_HIP(hipGetLastError());
    if (p.per) mix<MIX_LAMBDA_LOSS | MIX_PER>(p, YT, G, W, TDA);
    else mix<MIX_LAMBDA_LOSS>(p, YT, G);
    MQ_HIP(hipGetLastError());
  }
  if (p.per) {   // the new priorities of the batch's episodes, from the tail's |td m| record
    hipLaunchKernelGGL(per_priority_kernel, dim3((d.B + 3) / 4), dim3(256), 0, s, d, rp, (const float*)TDA,
                       h->per.prio, h->per.prio_max, h->per.n_prio, h->per.eps);
    MQ_HIP(hipGetLastError());
  }
  return MQ_OK;
}

// The two-layer hypernet behind the mixer tail's dHYP: layer 2's backward into dA1, then every hypernet weight and
// bias gradient as p.ns m-slices of slab_mix (reduce() sums them).
int Step::hypernet2_backward(const StepPlan& p) {
  if (!p.hyper2) return MQ_OK;
  pt.begin(PH_DWH);
  const Hyp2Lay& y = h->y2;
  Hyp2BwdProb pb{y, h->on, h->A1, w.dHYP, h->dA1, d.M, d.NH};
  MQ_HIP(launch_gemm(pb, d.M, y.N1, 1, s));
  const int t0 = (y.nE + GBM - 1) / GBM, t1 = (y.E + GBM - 1) / GBM, t2 = (y.N1 + GBM - 1) / GBM;
  Hyp2DwProb pw{y, h->A1, h->dA1, w.dHYP, w.S0, w.slab_mix, h->len_mix, h->off[MQ_P_HW1_W], d.M, d.NH, d.S, p.ns, t0, t1};
  MQ_HIP(launch_gemm(pw, (t0 + t1 + t2) * GBM, std::max(y.He, d.S), p.ns, s));
  return MQ_OK;
}

// BPTT, with dX1 / dW1 as GEMMs behind the unfused recurrence.
int Step::bptt(const StepPlan& p) {
  pt.begin(PH_GRUB);
  const float* P0 = h->on;
  const int64_t l1 = (int64_t)mq::H * d.I + mq::H;
  const size_t dyn = ((size_t)2 * d.A * mq::H + d.A) * sizeof(float);   // the one-row kernels' fc2 staging
  if (p.ffn) {
    // dP2 (in dGI's buffer, as [RT][H]) and the fc2-gradient slabs, then dP1, [dWr | dbr] and dW1 as GEMMs
    const size_t dyn2 = ffn_dp2_lds_bytes(d.A);
    MQ_LDS(ffn_dp2_kernel, dyn2);
    hipLaunchKernelGGL(ffn_dp2_kernel, dim3(p.ffn_nblk2), dim3(256), dyn2, s, d, rp, P0 + h->off[MQ_P_FC2_W],
                       (const float*)w.dch, (const float*)w.Hs, w.dGI, w.slab_rnn + ffn_w2_slabs(p), p.ffn_rpb);
    MQ_HIP(hipGetLastError());
    pt.begin(PH_DX1);
    {
      FfnDx1Prob px{w.dGI, P0 + h->off[MQ_P_FFN_W], w.X1, w.dP1, RT};
      MQ_HIP(launch_gemm(px, (int)RT, mq::H, 1, s));
    }
    pt.begin(PH_DW1);
    {
      FfnDwrProb pr{w.dGI, w.X1, w.slab_rnn, RT, p.ffn_wr_ns};
      MQ_HIP(launch_gemm(pr, mq::H, mq::H, p.ffn_wr_ns, s));
      Dw1Prob p1{d.I, w.dP1, w.XIN, w.slab_fc1, RT, p.dw1_ns};
      MQ_HIP(launch_gemm(p1, mq::H, d.I, p.dw1_ns, s));
    }
    return MQ_OK;
  }
  if (p.fwd == FWD_TILES) {
    // the two-role (chain / weight-gradient waves) BPTT, 512 threads
    dispatch_kq1(p.kq1, [&](auto K) {
      hipLaunchKernelGGL(gru_bwd_split_kernel<decltype(K)::value>, dim3(p.nblk_bwd), dim3(512), 0, s, d, rp, P0, L, w,
                         h->len_rnn, l1);
    });
    MQ_HIP(hipGetLastError());
  } else if (p.fused_bwd) {
    // one row per workgroup: dW_hh / dW_ih / dX1 / dW1 on the chain's idle matrix cores (gru_bwd_fused.hpp)
    if (p.dwh_in_bwd) {   // dW_hyper's tiles in this grid: the reduction's dW_hyper blocks, same geometry
      w.dwh_tj = p.tj;
      w.dwh_ns = p.ns;
      w.dwh_n = p.ndwh;
      w.dwh_len = h->len_mix;
    }
    // diagnostic (MQ_DIAG bwd_stamp=<file>): step stamps of the first 8 workgroups
    std::string bstamp_path;
    const bool bstamp = !p.dwh_in_bwd && env_item("MQ_DIAG", "bwd_stamp", &bstamp_path) && !bstamp_path.empty() &&
                        d.Tp <= BSTN - BSTH;
    if (p.lean) {
      if (p.dwh_in_bwd) MQ_LDS((gru_bwd_fused_kernel<1, false, kBwdLean>), dyn);
      else MQ_LDS((gru_bwd_fused_kernel<0, true, kBwdLean>), dyn);   // the larger of the two builds
    } else {
      if (p.dwh_in_bwd) MQ_LDS(gru_bwd_fused_kernel<1>, dyn);
      else MQ_LDS((gru_bwd_fused_kernel<0, true>), dyn);
    }
    if (p.dwh_in_bwd) launch_bwd_fused_dwh(dyn, s, d, rp, P0, L, w, h->pitch_rnn, l1, p.lean);
    else launch_bwd_fused(dim3(d.R), dyn, s, d, rp, P0, L, w, h->pitch_rnn, l1, p.lean, bstamp);
    if (bstamp) {
      std::vector<uint32_t> st((size_t)8 * BSTN);
      MQ_HIP(hipMemcpyAsync(st.data(), w.GI, st.size() * 4, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipStreamSynchronize(s));
      if (FILE* f = fopen(bstamp_path.c_str(), "ab")) { fwrite(st.data(), 4, st.size(), f); fclose(f); }
    }
    MQ_HIP(hipGetLastError());
  } else {
    int rc = MQ_OK;
    dispatch_rw<4>(p.rw_bwd, [&](auto K) {
      constexpr int RW = decltype(K)::value;
      rc = lds_fits((const void*)gru_bwd_kernel<RW>, dyn, ("gru_bwd_kernel<" + std::to_string(RW) + ">").c_str());
      if (rc == MQ_OK)
        hipLaunchKernelGGL(gru_bwd_kernel<RW>, dim3(p.nblk_bwd), dim3(512), dyn, s, d, rp, P0, L, w, h->len_rnn);
    });
    if (rc) return rc;
    MQ_HIP(hipGetLastError());
    pt.begin(PH_DX1);
    {
      Dx1Prob p{w.dGI, h->on + h->off[MQ_P_RNN_W_IH], w.X1, w.dP1, RT};
      MQ_HIP(launch_gemm(p, (int)RT, mq::H, 1, s));
    }
    pt.begin(PH_DW1);
    {
      const int ns = p.dw1_ns;
      Dw1Prob p{d.I, w.dP1, w.XIN, w.slab_fc1, RT, ns};
      MQ_HIP(launch_gemm(p, mq::H, d.I, ns, s));
    }
  }
  return MQ_OK;
}

// The slab reductions into the flat gradient buffer; pass 1 shares its launch with dW_hyper (dwh_red1_kernel) unless
// dW_hyper's tiles rode in the BPTT's grid.
int Step::reduce(const StepPlan& p) {
  const RedBuilder rb = plan_reduce(p, d, *h, w, h->grad);
  if (!rb.ok) return set_err(MQ_ERR_STATE, "step: more reduction regions than the plan holds");
  // pass-1 blocks would read slabs the dW_hyper blocks of the same grid still write
  if (p.dwh_in_red1 && !rb.mix_direct)
    return set_err(MQ_ERR_STATE, "dW_hyper fused with reduction pass 1 needs a direct slab region");
  if (p.dwh_in_red1) {
    pt.begin(PH_DWH);
    const int ndwh_pad = (p.ndwh + 15) / 16 * 16;
    hipLaunchKernelGGL(dwh_red1_kernel<4>, dim3(ndwh_pad + rb.b1), dim3(256), 0, s, d, L, (const float*)w.dHYP,
                       (const float*)w.S0, w.slab_mix, h->len_mix, p.ns, p.tj, p.ndwh, ndwh_pad, rb.pl);
    MQ_HIP(hipGetLastError());
    pt.begin(PH_RED);
  } else {
    pt.begin(PH_RED);
    if (rb.b1 > 0) {
      hipLaunchKernelGGL(red_pass1_kernel, dim3(rb.b1), dim3(256), 0, s, rb.pl);
      MQ_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(red_pass2_kernel, dim3(rb.b2), dim3(256), 0, s, rb.pl, w.norm_part);
  MQ_HIP(hipGetLastError());
  n_norm_part = rb.b2;
  pt.end();
  return MQ_OK;
}

}  // namespace
