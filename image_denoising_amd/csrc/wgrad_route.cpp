// The weight-gradient route (wgrad_route.h): eligibility, block / tile choice, stage shape and
// split policy of every weight-gradient launch, and the slab sizes that follow from them.
#include "dn_internal.h"

namespace dn {

int wgrad_taps(int mode) { return mode == W_C3 ? 9 : (mode == W_UP2 ? 4 : 1); }

bool wgrad_supported(int mode, int cout) {
  const int cf = (cout + 15) / 16;
  if (mode == W_C3 || mode == W_UP2) return cf == 3 || cf == 6;
  return mode == W_C1 && (cf == 1 || cf == 6);
}

WgradShape wgrad_shape(int mode, int N, int KH, int KW, int Cin, int Cout, int g_stride, int g_off,
                       int x_stride, int x_off, bool x6) {
  return WgradShape{mode, N, KH, KW, Cin, Cout, g_stride, g_off, x_stride, x_off,
                    Cin, 0, true, false, x6, 0};
}

int wgrad_split_policy(int slots, long wgs, long units, long row, bool group8) {
  long sp = slots / (wgs < 1 ? 1 : wgs);
  const long cap = (64L << 20) / (row < 1 ? 1 : row);  // <= 256 MB of slab
  if (sp > cap) sp = cap;
  // at least 2 pixel units per split: on the small levels the per-workgroup slab (up to 110 KB
  // written, then re-read by the reduction) outweighs the work of a 1-unit split
  if (sp > units / 2) sp = units / 2;
  // whole groups of 8 (k_wgrad1p's XCD map of the four parity blocks; splits past the pixel count
  // write zero rows)
  if (group8) sp = sp < 8 ? 8 : sp / 8 * 8;
  return (int)(sp < 1 ? 1 : sp);
}

namespace {

// K stage of the 3x3 kernels: 32-pixel row segments, or 16 / 8 / 4 pixels x 2 / 4 / 8 rows of
// narrow images
int stage_swl(int KW) { return KW >= 32 ? 5 : (KW >= 16 ? 4 : (KW >= 8 ? 3 : 2)); }

long ceil_div(long a, long b) { return (a + b - 1) / b; }

// Output-channel block of the blocked family.  3x3: 96 / 48 / 32; 1x1: 96 / 48.  Every block of
// one layer uses the same split count, so each slab row holds the whole [W ; b] image and one
// reduction job finishes it.
int gw_block(int mode, int cout) {
  if (mode == W_C3) return cout <= 32 ? 32 : (cout <= 48 ? 48 : 96);
  return cout <= 48 ? 48 : 96;
}

// input channels per workgroup of the blocked 3x3 kernels: 32 for 96-wide output blocks; for
// 32-wide blocks (RDB growth convs, 24-channel layers) 32 / 48 / 64, whichever pads Cin least
// (ties: the wider block, fewer workgroups re-reading the gradient operand); else 48
int gw_cin_t(int cb, int Cin) {
  if (cb == 96) return 32;
  if (cb == 48) return 48;
  int best = 48;
  long pad = 1L << 30;
  for (int t : {64, 48, 32}) {
    const long p = (long)(Cin + t - 1) / t * t;
    if (p < pad) { pad = p; best = t; }
  }
  return best;
}

}  // namespace

WgradRoute wgrad_route(const WgradShape& sh) {
  WgradRoute r{};
  r.sh = sh;
  r.par = 1;
  r.nz = 1;
  const int mode = sh.mode, Cin = sh.Cin, Cout = sh.Cout, KW = sh.KW, taps = wgrad_taps(mode);
  const bool c3 = mode == W_C3, up2 = mode == W_UP2;
  // operands are read as channel quads from 16-byte aligned pixels; every quad that starts inside
  // [0, C) must lie inside the view's row (reads past C land on padding or a neighbouring slice)
  const bool quads = !((sh.g_stride | sh.g_off | sh.x_stride | sh.x_off) & 3);
  const bool x_in = sh.x_off + ((Cin + 3) & ~3) <= sh.x_stride;
  const bool g_in = sh.g_off + ((Cout + 3) & ~3) <= sh.g_stride;
  // k_wgrad3p / k_wgrad3q address an image with 32-bit buffer offsets: under 2 GiB per operand
  const bool fits32 = (long)sh.KH * KW * sh.g_stride * 4 < 0x7fffffffL &&
                      (long)sh.KH * KW * sh.x_stride * 4 < 0x7fffffffL;
  r.swl = c3 ? stage_swl(KW) : 0;
  const long units_c3 = (long)sh.N * ceil_div(sh.KH, 32 >> r.swl) * ceil_div(KW, 1 << r.swl);
  const long units_row = (long)sh.N * sh.KH * ceil_div(KW, 32);  // one 32-pixel row segment per stage
  r.row = (long)Cout * sh.cin_total * taps + (sh.bias ? Cout : 0);
  // the 256 MB cap counts this launch's own [W ; b], whatever the row it is written into
  long cap_row = (long)Cout * Cin * taps + Cout, units = c3 ? units_c3 : units_row, wgs;
  int slots = 768;
  bool group8 = false;

  if (sh.blocked) {
    r.zc = gw_block(mode, Cout);
    r.nz = (int)ceil_div(Cout, r.zc);
    r.co_fr = r.zc / 16;
    r.cib = c3 ? gw_cin_t(r.zc, Cin) : 96;
    const bool ok = (c3 || mode == W_C1) && quads && x_in && g_in && Cin >= (c3 ? 16 : 1) &&
                    Cout >= 1 && !sh.head_gnb;
    if (!ok) {
      r.err = "no blocked weight-gradient kernel for this layer shape or these views";
    } else if (c3 && sh.x6 && KW >= 8) {  // the bf16x6 kernels stage rows >= 8 wide
      slots = 512;
      r.kernel = r.zc == 96 && Cin >= 32 && fits32 ? WK_WGRAD3P : WK_WGRAD3S;
    } else {
      r.kernel = c3 ? WK_WGRAD3 : WK_WGRAD1;
    }
    wgs = r.nz * ceil_div(Cin, r.cib);
  } else if (!c3 && Cin == Cout && (Cin == 96 || Cin == 48) && quads &&
             sh.g_off + Cout <= sh.g_stride && sh.x_off + Cin <= sh.x_stride &&
             sh.cin_total == Cin && !sh.ci_base && sh.bias) {
    // square 1x1 / deconv: k_wgrad1, or k_wgrad1p (bf16x6, 96 x 96; 32-bit offsets inside a
    // 32-pixel stage).  Deconv: one block of rows [W (ci, co) | b] per parity.
    const bool p1 = sh.x6 && Cout == 96 && 32L * sh.g_stride * 4 < 0x7fffffffL &&
                    32L * sh.x_stride * 4 < 0x7fffffffL;
    r.par = up2 ? 4 : 1;
    r.co_fr = Cout / 16;
    r.cib = Cin;
    r.row = cap_row = (long)Cout * Cin + Cout;
    group8 = up2;
    wgs = r.par;
    // head_gnb (g = nb, the gradient recomputed from at most 4 nin_c outputs): k_wgrad1p only
    if (sh.head_gnb && !(p1 && !up2 && sh.head_gnb > 0 && sh.head_gnb <= 4 && sh.g_stride == 96 &&
                         !sh.g_off))
      r.err = "the head's recomputed gradient needs k_wgrad1p on compact 96-channel views";
    else
      r.kernel = p1 ? WK_WGRAD1P : WK_WGRAD1;
  } else {
    const int cf = (Cout + 15) / 16;
    r.co_fr = cf;
    // the asynchronous 3x3 kernels: 96 or 48 outputs, Cin >= 32 (a 32/48-channel block would be
    // mostly padding)
    const bool async3 = c3 && (Cout == 96 || Cout == 48) && Cin >= 32 && quads && x_in;
    // input channels per workgroup that the split count is planned for: k_wgrad3's / k_wgrad3s's /
    // k_wgrad3p's for every 3x3 launch, so one slab plan serves k_wgrad (16 per workgroup) too
    int pr = 1, pc = 32;
    if (c3) r.cib = cf >= 6 ? 32 : 48;
    else if (up2) { r.cib = 16; pc = 16; }
    else { r.cib = cf == 1 ? 32 : 96; pr = cf >= 6 ? 1 : 2; }
    if (!c3) units = (long)sh.N * ceil_div(sh.KH, pr) * ceil_div(KW, pc);
    wgs = ceil_div(Cin, r.cib);
    if (sh.head_gnb) {
      r.err = "the head's recomputed gradient needs k_wgrad1p on compact 96-channel views";
    } else if (async3 && sh.x6 && KW >= 8) {
      slots = 512;
      // 48 -> 48 takes the 4-wave k_wgrad3q on rows >= 128 wide, the 3-wave k_wgrad3p below
      r.kernel = !fits32 ? WK_WGRAD3S : (Cout == 48 && KW >= 128 ? WK_WGRAD3Q : WK_WGRAD3P);
    } else if (async3) {
      r.kernel = WK_WGRAD3;
    } else if (wgrad_supported(mode, Cout)) {
      r.kernel = WK_WGRAD;
      if (c3) r.cib = 16;
    } else {
      r.err = "no weight-gradient kernel for this Cout";
    }
  }
  // k_wgrad3p / k_wgrad3q stage rows of at most 16 pixels (2 rows of 16: 72 X pixels per stage
  // instead of 102 for one row of 32)
  if ((r.kernel == WK_WGRAD3P || r.kernel == WK_WGRAD3Q) && r.swl > 4) r.swl = 4;
  r.splits = wgrad_split_policy(slots, wgs, units, cap_row, group8);
  r.floats = (long)r.par * r.splits * r.row;
  return r;
}

WgradSize wgrad_size(int mode, int N, int KH, int KW, int Cin, int Cout, bool blocked) {
  WgradSize z{0, 0};
  const int gs = (Cout + 3) & ~3, xs = (Cin + 3) & ~3;
  for (int aligned = 0; aligned < 2; ++aligned)
    for (int x6 = 0; x6 < 2; ++x6) {
      WgradShape sh = wgrad_shape(mode, N, KH, KW, Cin, Cout, gs + !aligned, 0, xs + !aligned, 0,
                                  x6 != 0);
      sh.blocked = blocked;
      const WgradRoute r = wgrad_route(sh);
      if (r.par * r.splits > z.rows) z.rows = r.par * r.splits;
      if (r.floats > z.floats) z.floats = r.floats;
    }
  return z;
}

}  // namespace dn
