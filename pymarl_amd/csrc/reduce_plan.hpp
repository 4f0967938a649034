// The slab reductions of one train step (optim_kernels.hpp red_pass1_kernel / red_pass2_kernel) as a plan: a pure
// function of the step's plan, its shapes, the parameter layout and the workspace pointers. No HIP call: the launches
// are Step::reduce's (step_launch.hpp) and launch_reduce's (optim_host.hpp), and tests/host/ws_probe.cpp reads off it
// what a step asks of red_tmp and norm_part.
#pragma once
#include "learner_layout.hpp"

namespace mq {

// Norm partials (pass 2's blocks) a norm_part buffer of fixed size holds: the COMA and actor-critic workspaces'
// tables and launch_reduce's check (optim_host.hpp) share it.
constexpr int kNormPartMax = 4096;

// Regions in gradient order, then the loss sums (not part of the norm).
struct RedBuilder {
  RedPlan pl{};
  int b1 = 0, b2 = 0;   // blocks of pass 1 / pass 2 (pass 2 writes one norm_part float per block)
  float* tmp;
  bool mix_direct = false;   // plan_reduce: dW_hyper's slabs go straight to pass 2
  bool ok = true;            // cleared by a region past kRedMaxRegions: nothing was written for it, launch nothing
  explicit RedBuilder(float* t) : tmp(t) {}
  // returns true when the region is summed by pass 2 straight from its slabs (no pass-1 blocks read them)
  bool add(const float* src, int nslab, int64_t len, float* dst, bool sq, int64_t pitch = 0, bool direct_ok = false,
           int perm = 0) {
    if (len <= 0 || nslab <= 0) return false;
    if (pl.nr >= kRedMaxRegions) return ok = false;
    RedRegion& R = pl.r[pl.nr++];
    R.src = src; R.dst = dst; R.len = len; R.pitch = pitch > 0 ? pitch : len; R.nslab = nslab; R.sq = sq ? 1 : 0;
    R.perm = perm;
    if (direct_ok && nslab <= kRedZ) {   // pass 2 sums the slabs themselves: no pass-1 blocks, no tmp
      R.zc = 1; R.ng = nslab; R.tmp = (float*)src; R.tpitch = R.pitch; R.vec = 0; R.xcd = 0;
      R.blk1 = b1;
      R.blk2 = b2; b2 += (int)((len + 255) / 256);
      return true;
    }
    R.tpitch = len;
    // at most kRedZ groups, so pass 2 sums <= 16 partials per element with all loads in flight
    R.zc = (nslab + kRedZ - 1) / kRedZ;
    R.ng = (nslab + R.zc - 1) / R.zc;
    R.tmp = tmp;
    tmp += R.ng * len;
    R.vec = (len % 4 == 0 && R.pitch % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)R.tmp & 15) == 0) ? 1 : 0;
    R.xcd = (nslab % 128 == 0 && R.ng == kRedZ && b1 % 16 == 0) ? 1 : 0;
    const int nb = (int)((len + 255) / 256), nb1 = R.vec ? (int)((len + 1023) / 1024) : nb;
    R.blk1 = b1; b1 += nb1 * R.ng;
    R.blk2 = b2; b2 += nb;
    return false;
  }
};

// feed-forward agent: slab_rnn holds the step's [dWr | dbr] split-K slabs, then ffn_dp2_kernel's [dW2 | db2] slabs
inline int64_t ffn_w2_slabs(const StepPlan& p) { return (int64_t)p.ffn_wr_ns * FfnDwrProb::LEN; }

// The step's regions into the flat gradient buffer `grad` ([P | MQ_NSUMS]).
inline RedBuilder plan_reduce(const StepPlan& p, const Dims& d, const Layout& y, const Work& w, float* grad) {
  RedBuilder rb(w.red_tmp);
  rb.add(w.slab_fc1, p.nsplit_fc1, (int64_t)H * d.I + H, grad + y.off[MQ_P_FC1_W], true);
  if (p.ffn) {   // [rnn.w | rnn.b] from the split-K slabs, [fc2.w | fc2.b] from ffn_dp2_kernel's
    rb.add(w.slab_rnn, p.ffn_wr_ns, FfnDwrProb::LEN, grad + y.off[MQ_P_FFN_W], true);
    rb.add(w.slab_rnn + ffn_w2_slabs(p), p.ffn_nblk2, (int64_t)d.A * H + d.A, grad + y.off[MQ_P_FC2_W], true);
  } else if (p.fused_bwd) {   // [W_ih | W_hh] in the BPTT's C-tile order (red_dst), then the biases and fc2
    const int64_t lm = 2LL * G3 * H;
    rb.add(w.slab_rnn, p.nblk_bwd, lm, grad + y.off[MQ_P_RNN_W_IH], true, y.pitch_rnn, false, 1);
    rb.add(w.slab_rnn + lm, p.nblk_bwd, y.len_rnn - lm, grad + y.off[MQ_P_RNN_W_IH] + lm, true, y.pitch_rnn);
  } else {
    rb.add(w.slab_rnn, p.nblk_bwd, y.len_rnn, grad + y.off[MQ_P_RNN_W_IH], true);
  }
  if (d.mixer == MQ_MIXER_QMIX) {
    // dW_hyper's few m-slice slabs go straight to pass 2 (they are written in the same launch as pass 1)
    rb.mix_direct = rb.add(w.slab_mix, p.nsplit_mix, y.len_mix, grad + y.off[MQ_P_HW1_W], true, 0, true);
    rb.add(w.slab_v2, p.nblk_mix, d.E + 1, grad + y.off[MQ_P_V2_W], true);
  }
  rb.add(w.loss_part, p.nblk_mix, MQ_NSUMS, grad + y.P, false);
  return rb;
}

}  // namespace mq
