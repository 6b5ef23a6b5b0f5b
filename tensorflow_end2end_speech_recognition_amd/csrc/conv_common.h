// What the two convolution files share: the tap geometry and the epilogue gate of the implicit-GEMM kernels, and the
// launchers of the tiled kernels (conv.hip) that the 3x3 entry points (conv3x3.hip) fall back to when their
// image-resident forms do not apply.
#pragma once
#include "common.h"

// Tap geometry of the implicit kernels: KW columns per row, and the (row, column) origin (OY, OX) of tap 0, i.e. tap t
// reads the pixel shifted by (t / KW - OY, t % KW - OX).  3x3 and 3x5 SAME: origin (1, 1) / (1, 2) for the forward and
// for the flipped data-gradient image alike (odd widths are symmetric); 3x4 SAME (TensorFlow pads one column before and
// two after): origin (1, 1) forward, (1, 2) for the flipped image.
template <int KH_, int KW_, int OY_, int OX_>
struct Taps {
  static constexpr int KH = KH_, KW = KW_, OY = OY_, OX = OX_, N = KH_ * KW_;
};
typedef Taps<3, 3, 1, 1> Taps33;
typedef Taps<3, 5, 1, 2> Taps35;
typedef Taps<3, 4, 1, 1> Taps34f;
typedef Taps<3, 4, 1, 2> Taps34b;

struct ConvGate {               // epilogue operands of act == 2 (data gradient) / act == 3 (forward)
  const bf16_t* act;            // act == 2: ReLU output of the layer below, [pixels, Cout of this product]
  float keep;
  uint64_t seed, offset;        // dropout applied to that output (element e -> Philox block offset + e / 4, asr_dropout_apply)
  int use_drop;                 // act == 2: 0 = ReLU gate only, 1 = form the mask (Philox), 2 = `act` is the DROPPED output:
};                              //           it is > 0 exactly where the unit was active AND kept, scale 1 / keep there
typedef __attribute__((ext_vector_type(4))) unsigned short cg_us4_t;
// (the gate operand of act == 2 as a separate load: the image-resident kernel requests it at the top of a pixel tile, a
// thousand matrix cycles ahead of the epilogue that consumes it)
__device__ __forceinline__ cg_us4_t conv_gate_load(const ConvGate& gate, size_t e) {
  return *reinterpret_cast<const cg_us4_t*>(gate.act + e);
}
// act: 0 none, 1 ReLU, 2 gate by the layer below (v = act > 0 ? v * mask : 0) -- the ReLU / dropout backward of the layer
// BELOW in the epilogue of the data gradient, instead of an fp32 gradient that asr_relu_bwd(_drop) would read back --,
// 3 (forward) ReLU, round to bf16, then tf.nn.dropout: the stored activation is the dropped one, bit for bit what
// asr_dropout_apply makes of the stored ReLU output, and the undropped one is never written
__device__ __forceinline__ void conv_gate_apply(int act, const ConvGate& g, size_t e, float (&v)[4]) {
  if (act == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  } else if (act == 2) {
    const cg_us4_t a = conv_gate_load(g, e);
    float mk[4] = {1.f, 1.f, 1.f, 1.f};
    if (g.use_drop == 1) asr_dropout_words(g.offset + e / 4, g.seed, g.keep, 1.f / g.keep, mk);
    else if (g.use_drop == 2) { const float inv = 1.f / g.keep; mk[0] = mk[1] = mk[2] = mk[3] = inv; }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = bf16_to_f32(a[r]) > 0.f ? v[r] * mk[r] : 0.f;
  } else if (act == 3) {
    float mk[4];
    asr_dropout_words(g.offset + e / 4, g.seed, g.keep, 1.f / g.keep, mk);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = bf16_to_f32(f32_to_bf16(fmaxf(v[r], 0.f))) * mk[r];
  }
}

// ---- conv.hip: the tiled kernels of any geometry (defined for Taps33 / Taps35 / Taps34f / Taps34b)
// out = act(conv(x) + bias): the forward, or the data gradient when x = dOut and wt = the flipped-tap image (Cin / Cout are
// then the layer's Cout / Cin); `what` names the caller in error messages
template <typename TP>
int asr_conv_nt(asr_handle* h, const char* what, const void* x, int N, int H, int W, int Cin, const void* wt,
                const float* bias, int Cout, int act, const ConvGate& gate, bool out_f32, void* out, asr_stream s);
// the two weight images (forward, flipped) of a kh x kw filter with ntaps = kh kw taps from the HWIO fp32 master
int asr_conv_prep(asr_handle* h, const char* what, int ntaps, const float* w_hwio, int Cin, int Cout, void* wt_fwd,
                  void* wt_bwd, asr_stream s);
// Weight gradient = pixel-range slabs in the scratch arena + a fixed-order sum of the slabs.  The plan: *S slabs of *kchunk
// pixels (a multiple of 64) for `tiles` output tiles of slab_bytes per slab -- ~2048 workgroups in all, at least 512 pixels
// per slab, at most max_slabs, as many as the arena holds
int asr_conv_wgrad_plan(asr_handle* h, const char* what, int Mpix, int tiles, size_t slab_bytes, int max_slabs, int* S,
                        int* kchunk);
// slab z = pixels [z kchunk, (z + 1) kchunk) -> partial[z][ntaps Cin][Cout] (128 x 128 tiles, [column][pixel] LDS image)
template <typename TP>
void asr_conv_wgrad_tiled(const void* x, const void* dy, int Mpix, int H, int W, int Cin, int Cout, int S, int kchunk,
                          float* partial, hipStream_t st);
// conv3x3.hip: the ASR_CONVP_PAIR_* counter of a Cin -> Cout product (asr_conv_path_counts)
int asr_conv_pair_counter(int Cin, int Cout);
// dw[i] (+)= sum_{z = 0 .. S-1} partial[z][i], slabs added in index order
void asr_conv_slab_sum(const float* partial, int S, size_t total, float* dw, int accumulate, hipStream_t st);
