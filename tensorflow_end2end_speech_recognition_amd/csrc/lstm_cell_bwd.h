// The backward of one LSTMBlockCell element of the attention decoder, shared by every kernel that runs it: the plain
// launch and the fused query-FC + cell kernel of attention.hip (the backward loop of dec_loop.hip issues both), and the
// dx + cell kernel of a decoder stack (dec_stack.hip).  One statement of the arithmetic, so that the three agree bit for bit.
#pragma once
#include "common.h"

// What a cell backward reads and writes for one decoder step of one layer ([B,U] rows unless noted): the carried
// gradients dc_next / dh_next (+ dh_next2 with row stride ld2: the h-columns of the next step's cell-input gradient),
// the forward's gates [B,4U], raw cell state and previous cell state, peepholes [3,U] or NULL, live [B], the output
// dropout mask or NULL; dpre [B,4U], the carried gradients for the step before, dpeep_rows [B,3U] or NULL.
// clip > 0: a state the forward clamped passes nothing back (asr_lstm_cell_bwd_ex); 0 is the decoder's straight-through.
struct CellBwdArgs {
  const float *dc_next, *dh_next, *dh_next2, *gates, *c_raw, *c_prev, *peep, *live, *use_mask;
  float *dpre, *dc_prev, *dh_prev_carry, *dpeep_rows;
  int ld2;
  float clip;
};

struct CellBwdElem {
  float d_i, d_g, d_f, d_o, dc_prev;
};

// dh: gradient w.r.t. the cell's raw output h (masked cell-output gradient + carried dh); i, g, f, o: post-activation
// gates; c / cp: new (raw) and previous cell state; wci / wcf / wco: peepholes (0 without)
__device__ __forceinline__ CellBwdElem lstm_cell_bwd_elem(float dh, float dc_next, float i, float g, float f, float o,
                                                          float c, float cp, float wci, float wcf, float wco, float clip) {
  CellBwdElem r;
  const float tc = tanhf(c);
  r.d_o = dh * tc * o * (1.f - o);
  const float dct = dc_next + dh * o * (1.f - tc * tc) + r.d_o * wco;
  const float dc = (clip > 0.f && fabsf(c) >= clip) ? 0.f : dct;     // a clamped state passes nothing back
  r.d_g = dc * i * (1.f - g * g);
  r.d_i = dc * g * i * (1.f - i);
  r.d_f = dc * cp * f * (1.f - f);
  r.dc_prev = dc * f + r.d_i * wci + r.d_f * wcf;
  return r;
}

// host side: the plain cell backward launch with every operand of CellBwdArgs (attention.hip), for the loops of other files
int asr_lstm_cell_bwd_args(asr_handle* h, const float* dh_use, const CellBwdArgs& c, int B, int U, asr_stream s);

// decoder stack, backward step k (dec_stack.hip): the cell-backward operands of upper layer l >= 1 (cur: which of the
// layer's two carried-gradient buffers holds step k+1's), and the launch(es) of lower layer l (0 .. L-2): the dx product of
// layer l+1 with layer l's cell backward (operands ca) behind it
CellBwdArgs asr_stack_cell_args(const asr_att_decoder* a, const asr_att_stack* sk, int l, int k, int cur);
int asr_stack_dec_bwd_lower(asr_handle* h, const asr_att_decoder* a, const asr_att_stack* sk, int l, int k,
                            const CellBwdArgs& ca, asr_stream s);
