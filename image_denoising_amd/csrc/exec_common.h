// What the host executors (unet.cpp, resnet.cpp, iunet.cpp) share (internal): the error macros,
// the backward's streams, the op helpers, and what the UNet and the RESNET have in common (slab
// plan, 3x3 data-gradient routes, dec_conv1a's weight gradient, the nin head): exec_common.cpp.
#pragma once
#include <functional>
#include <string>

#include "../../include/denoise_hip.h"
#include "dn_internal.h"

namespace dn {

void set_error(const std::string& s);
extern thread_local std::string g_last_error;

// in a function returning dn_status: a failed HIP call sets the thread's message and returns
#define DN_TRY(x)                                                         \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      ::dn::set_error(std::string("HIP error in ") + #x + ": " + hipGetErrorString(e_)); \
      return DN_ERR_HIP;                                                  \
    }                                                                     \
  } while (0)
// DN_TRY(call) bracketed by an OpTimer (statement form)
#define DN_TIMED(st, op, flops, K, NO, h, w, n, call)          \
  do {                                                        \
    const ::dn::OpTimer dn_timer_(st, op, flops, K, NO, h, w, n); \
    DN_TRY(call);                                             \
  } while (0)

// what a plan's *_debug_buffers hands out per activation / gradient buffer: offset in floats,
// pixel stride in channels, resolution level
using BufferVisitor = std::function<void(long off, int stride, int level)>;

struct Layer {
  int cout, cin, k;
  bool deconv;   // ConvTranspose2d: weight [cin][cout][2][2]
  long woff;     // float offset of the weight in the flat buffer (bias follows)
  long wcount;
};

// The backward's side streams: weight gradients on `st`, slab reductions on `rst`, with their
// fork / join events; one set per host thread and device (nullptr when creating them failed: run
// on one stream).
struct SideStream {
  hipStream_t st = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  // the slab reductions' own stream (round 6): a flush there overlaps both the data-gradient
  // chain and the remaining weight gradients instead of delaying the latter on `st`
  hipStream_t rst = nullptr;
  hipEvent_t rfork = nullptr, rjoin = nullptr;
};
SideStream* side_stream(hipStream_t s);
bool bwd_two_streams();  // false under DN_BWD_STREAMS=0: the backward on one stream
// the side stream continues after the work queued on s so far (side == nullptr: nothing to do)
hipError_t side_fork(SideStream* side, hipStream_t s);

// The streams of one backward pass and its queued slab reductions.  The weight gradients only
// read what nothing later in the backward rewrites and write their own slabs, so they overlap the
// data-gradient chain: each is forked from the caller's stream after the kernel that produced its
// gradient, and the branches are joined at the end.  (DN_BWD_STREAMS=0 or launch profiling, where
// an event pair must bracket one kernel alone: side == nullptr and s2 == s.)
struct BwdStreams {
  SideStream* side;
  hipStream_t s, s2;  // the caller's stream (data gradients); the weight gradients' stream
  RedBatch rb;        // every weight gradient's reduction, launched in batches
  explicit BwdStreams(hipStream_t stream);
  hipError_t fork() { return side_fork(side, s); }
  // the reductions queued so far on the reduction stream, behind the weight gradients queued on
  // s2 so far; one stream: nothing, they stay queued for the pass's last red_flush on s
  hipError_t flush_reductions();
  // s continues after the weight gradients and (reductions) the reduction stream's work
  hipError_t join(bool reductions = true);
};

// ---- op helpers ----
// zc of the bf16x6 data gradient of a 3x3 layer producing nout channels (0: one block)
int x6_dgrad_zc(int nout);
WView conv_fwd_view(const float* w, int K, int ksize);
WView conv_dgrad_view(const float* w, int cin_total, int ksize);
WView deconv_fwd_view(const float* w, int cout);
WView deconv_dgrad_view(const float* w, int cout);
long conv_fwd_pack_size(int K, int cout, int ksize);
long conv_dgrad_pack_size(int cout, int nout, int ksize);
long deconv_fwd_pack_size(int cin, int cout);
long deconv_dgrad_pack_size(int cout, int cin);
hipError_t pack_conv_fwd(const float* w, int K, int cout, int ksize, float* out, hipStream_t s);
hipError_t pack_conv_dgrad(const float* w, int cin_total, int nout, int cout, int ksize, float* out,
                           hipStream_t s);
hipError_t pack_deconv_fwd(const float* w, int cin, int cout, float* out, hipStream_t s);
hipError_t pack_deconv_dgrad(const float* w, int cout, int cin, float* out, hipStream_t s);
hipError_t conv_forward(const View& in, int N, int H, int W, int K, const float* wp,
                        const float* b, int cout, int ksize, int act, const View& out,
                        int out_layout, hipStream_t s);
hipError_t conv_dgrad(const View& dz, int N, int H, int W, int cout, const float* wp, int nout,
                      int ksize, int epi, const View& mask, const View& dx, hipStream_t s);
hipError_t deconv_forward(const View& x, int N, int h, int w, int cin, const float* wp,
                          const float* b, int cout, const View& out, hipStream_t s);
hipError_t deconv_dgrad(const View& dy, int N, int h, int w, int cout, const float* wp, int cin,
                        const View& mask, int epi, const View& dx, hipStream_t s);
// nin_b's weight gradient only (WgradArgs::head_gnb, hd_*): the gradient operand recomputed from
// nb and dy, nin_c's weight gradient formed from the same reads
struct WgradHead {
  int gnb; const float* dy; int dy_stride; const float* wc;
  float* slab_c; float* dwc;
};
// The one weight-gradient launch sequence: fills WgradArgs from the route and the operand
// pointers (g, x: the origins of the route's views), takes the launch profiler's record, launches
// the route's kernel and queues its reductions into dwb = [W | b].  slab: [64 floats | the route's
// rows]; zeros == nullptr: the 64 floats are zeroed here and serve as the DMA padding; rb: the
// reductions are queued, not launched.  A route without a kernel is DN_ERR_ARG with its reason.
dn_status wgrad_run(const WgradRoute& r, const float* g, const float* x, float* dwb, float* slab,
                    const float* zeros, hipStream_t s, RedBatch* rb = nullptr,
                    const WgradHead* head = nullptr);
// the route of the fixed family's usual launch from its two views
inline WgradRoute wgrad_route(int mode, const View& g, const View& x, int N, int KH, int KW,
                              int cout, int cin, bool x6) {
  return wgrad_route(wgrad_shape(mode, N, KH, KW, cin, cout, g.stride, g.off, x.stride, x.off, x6));
}

// ---- the UNet's and the RESNET's common pieces ----
// One layer's weight-gradient slab of a with-backward plan: its split count and the floats behind
// the slab's 64 leading ones.  KH x KW: the grid its weight gradient runs over; C: in_nc.
enum SlabKind {
  SLAB_CONV,       // wgrad_run(): 3x3, 1x1 or deconv (mode W_C3 / W_C1 / W_UP2)
  SLAB_ENC0,       // launch_enc0_wgrad
  SLAB_D1A,        // d1a_wgrad: the MFMA kernel's rows, then the thin kernel's input-slice rows
  SLAB_NINC_THIN,  // launch_wgrad_thin, or the rows nin_b's k_wgrad1p<., GNB> writes for nin_c
};
struct WgradSlab { int splits; long floats; };
WgradSlab plan_wgrad_slab(int kind, int mode, int N, int KH, int KW, const Layer& L, int C);

// The kernel and weight image of a 3x3 (fp32: also 1x1) conv launch, decided once per pass: the
// pack loop writes the image the launch reads.  An executor may number further kinds from CV_END.
enum ConvKind { CV_F32, CV_X6, CV_END };  // the fp32 kernel | the bf16x6 kernels
struct ConvRoute {
  int kind;
  long img;           // workspace offset (floats) of the weight image
  int zc; long wp_z;  // CV_X6 data gradients: the zc-blocked image
  int tail;           // CV_X6: x6_image_mode
};
// layer L's data gradient (nout channels of its input) on an h x w grid; img_x6 < 0: no bf16x6 image
ConvRoute dgrad_route(bool x6, long img_f32, long img_x6, int N, int h, int w, const Layer& L,
                      int nout);
hipError_t pack_dgrad(PackBatch& pb, const ConvRoute& r, const float* w, const Layer& L, int nout,
                      float* ws, hipStream_t s);
// dz (L.cout channels) -> dx = channels [0, nout) of the layer's input, through epi / mask
hipError_t run_dgrad(const ConvRoute& r, const float* ws, const View& dz, int N, int h, int w,
                     const Layer& L, int nout, int epi, const View& mask, const View& dx,
                     hipStream_t s);

// the nin head's images into the pass's pack batch: nin_a | nin_b (forward), nin_b^T | nin_a^T
// followed by the weight gradients' 64 zero floats (backward); x6: the bf16x6 head kernels'
hipError_t pack_head_fwd(PackBatch& pb, bool x6, const float* wa, const float* wb, float* img,
                         hipStream_t s);
hipError_t pack_head_bwd(PackBatch& pb, bool x6, const float* wa, const float* wb, float* img,
                         float* zeros, hipStream_t s);

// nin_a .. nin_c of the flat parameters prm (each bias behind its weight), the images at img
HeadArgs head_args(const float* prm, const Layer& na, const Layer& nb, const Layer& nc,
                   const float* img, float* y);
// nin_a -> nin_b -> nin_c in one launch on the activated dec_conv1b output d1b [N, H, W, 96]
dn_status head_forward(const HeadArgs& h, const float* d1b, int N, int H, int W, bool x6,
                       hipStream_t s);

// the full-resolution tail of a backward pass; x6: weight gradients in the bf16x6 arithmetic
struct TailShape { int N, H, W; bool x6; const float* zeros; };
// a layer's [W | b] range of dparams, its slab and the rows its plan reserved (plan_wgrad_slab)
struct WgradDst { float* dwb; float* slab; int splits; };
// The head's backward: nin_c -> nin_b -> nin_a data gradients in one kernel (g_nb, g_na, g_d1b),
// then the three 1x1 weight gradients, each forked.  h: the network's buffers, image and NHWC dy.
// head_x6: k_head_bwd_x6; nin_b's weight gradient (k_wgrad1p<., GNB>) then recomputes g_nb from nb
// and dy (384 B per pixel less than a stored one) and, at out_nc == 1, forms nin_c's as well.
dn_status head_backward(BwdStreams& bs, const TailShape& t, HeadBwdArgs h, bool head_x6,
                        const WgradDst& nina, const WgradDst& ninb, const WgradDst& ninc);
// dec_conv1a's weight gradient: the MFMA kernel over the first c1k - C channels of c1, the thin
// kernel over the network input (xin, NCHW); own slab rows each, own columns of W[co][c1k][9]
dn_status d1a_wgrad(BwdStreams& bs, const TailShape& t, const float* g_d1a, const View& c1,
                    int c1k, const float* xin, int C, const WgradDst& d);

}  // namespace dn
