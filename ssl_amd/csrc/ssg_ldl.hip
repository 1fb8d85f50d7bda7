// LDL's artifact map and the loss built on it (Details or Artifacts, CVPR 2022), on the GPU:
// GAN-Based-SR/basicsr/losses/loss_util.py:106-161 (get_local_weights, get_artifact_map, get_refined_artifact_map) and
// its callers ldlssl_model.py:220-224 / realesrgan_model.py:222-226:
//   pixel_weight = get_refined_artifact_map(gt, output, output_ema, 7); L1Loss(pixel_weight * output, pixel_weight * gt).
//
// Contract (o = output, g = GT, e = EMA output, each (B,C,H,W) fp32):
//   r = sum_c |g - o|, r_e = sum_c |g - e|                  (B,1,H,W), channels summed in order c = 0, 1, ...
//   P_b = var_unbiased(r_b over H*W) ^ (1/5)                one value per image
//   V_p = unbiased variance (/(k^2 - 1)) of the k x k window of r, reflect-padded by (k-1)/2, centred on p
//   w_p = P_b * V_p, set to 0 where r_p < r_e,p (strict; the refined variant only -- without e nothing is masked)
//   loss = lambda * mean |w*o - w*g| (or the sum), the two products rounded separately in fp32 like the reference's
// Gradient with respect to o only (GT and EMA carry none in both callers), sgn(0) = 0 everywhere:
//   direct        lambda/N sgn(w*o - w*g) w
//   dL/dw_p       lambda/N sum_c sgn(w*o - w*g)(o - g), zero where w_p was masked
//   dL/dV_p       dL/dw_p P_b;  dL/dP_b = sum_p dL/dw_p V_p
//   dV_p/dr_q     2 (r_q - mu_p) / (k^2 - 1), once for every window tap whose reflected source is q
//   dP_b/dr_q     1/5 var^(-4/5) 2 (r_q - mean_b) / (HW - 1)
//   dr_q/do_c,q   sgn(o - g)
// An image whose residual is constant (output == GT) has var = 0: the reference's pow backward then forms
// 0 * inf = NaN, and so does this file -- that image's whole gradient is NaN, as in the reference.
//
// Three launches per call, no float atomics, no scatter (every sum has a fixed order: bit-reproducible):
//   ldl_residual  one thread per pixel (4 per thread): r, the mask bit (kept as the sign bit of the stored r: r >= 0,
//                 a masked r = +0 is stored as -0), and per-block fp64 partials of sum x, sum x^2 with x = r - r(pixel 0)
//                 of the image (the shift keeps a constant image's variance exactly 0 and the sums well conditioned).
//   ldl_map       one workgroup per 32 x 16 tile: r and its (k-1)/2 reflect halo in LDS, V_p in two passes (mean, then
//                 squared deviations), w, the loss terms and a_p = sum_c sgn(w o - w g)(o - g) (or the caller's
//                 upstream dL/dw); writes w, G = a P and G mu and one fp64 partial {sum |w o - w g|, sum a V} per tile.
//   ldl_grad      one workgroup per tile, the backward as a GATHER: pixel q sums G (r_q - mu_p) over the windows that
//                 contain it, each counted with its reflect multiplicity (separable: a row pass into LDS, then a column
//                 pass), adds the per-image P term and writes dL/do for every channel; workgroup (0,0) also folds the
//                 loss from the tile partials.
// get_local_weights alone (ssg_local_variance): ldl_map / ldl_grad on the caller's residual planes, P = 1, no mask.
// Compiled with -ffp-contract=off (csrc/Makefile): w*o - w*g must not become an fma (a rounded-product tie decides
// the sign the reference sees).
// Conditioning (measured against an fp64 evaluation, profiles/ldl_fp64_parity.txt): w, loss and gradient stay within
// about 1e-6 of their maximum in the callers' regime and within 5e-6 at mean(r) / std(r) = 30; the gather's
// r_q sum G - sum G mu loses digits in proportion to that ratio and crosses 1e-5 near 100 (4e-5 at 300 to 500).
#include "ssg_pixel.hpp"

namespace ssg {
namespace ldl {

using namespace pixel;                   // NT, sgnf, the 32 x 16 tile of ldl_map / ldl_grad and its reflect halo

constexpr int RES_PX = 4;                // pixels per thread in ldl_residual

enum Mode : int { LOSS = 0, MAP = 1, LOCALVAR = 2 };

struct Args {
  const float *o, *g, *e;   // (B,C,H,W)
  const float *rsrc;        // stored residuals (sign bit = mask) or, LOCALVAR, the caller's residual planes
  float *rs;                // ldl_residual's output: the stored residuals (B,H,W)
  const float *up;          // MAP: dL/dw (B,1,H,W); LOCALVAR: dL/dV; nullable
  float *w;                 // MAP / LOSS: w; LOCALVAR: V; nullable
  float *G, *GM;            // (B,H,W): a P and a P mu
  double2 *p1;              // (B, nb1) {sum x, sum x^2}
  double2 *p2;              // (B, ntile) {sum |w o - w g|, sum a V}
  float *grad;              // (B,C,H,W) dL/do, or LOCALVAR (B,1,H,W) dL/dr
  float *loss;              // LOSS: 1 float
  float scale;              // multiplies the gradient (LOSS: lambda / N or lambda)
  double loss_scale;        // LOSS: loss = loss_scale * sum |w o - w g|
  int B, C, H, W, k, nb1, tiles_x, ntile;
};

// r = sum_c |g - o| in channel order (torch.sum over dim 1 of small C accumulates c = 0, 1, ... in turn)
__device__ __forceinline__ float resid(const float *o, const float *g, size_t at, int C, int HW) {
  float r = fabsf(g[at] - o[at]);
  for (int c = 1; c < C; ++c) r += fabsf(g[at + (size_t)c * HW] - o[at + (size_t)c * HW]);
  return r;
}

// how often source sample p (0 <= p < n) sits in the window of radius R around q under reflect padding:
// padded positions q, -q (if q != 0) and 2(n-1) - q (if q != n-1) all hold sample q
__device__ __forceinline__ int mult(int q, int p, int n, int R) {
  return (abs(q - p) <= R) + (q != 0 && p + q <= R) + (q != n - 1 && 2 * (n - 1) - q - p <= R);
}

// fixed-order workgroup sum of two fp64 values (every thread gets the result; every thread must call it).  Not
// pixel::block_sum twice: it opens with a barrier because image_stats calls it back to back on one buffer.
__device__ __forceinline__ double2 block_sum2(double a, double b, double2 *sh) {
  __syncthreads();   // sh may still be read by a previous call
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = make_double2(a, b);
  __syncthreads();
  double2 s = sh[0];
  for (int i = 1; i < NT / 64; ++i) {
    s.x += sh[i].x;
    s.y += sh[i].y;
  }
  return s;
}

struct ImageStats {
  double mean, pc;   // pc: dL/dP 1/5 var^(-4/5) 2/(HW - 1) (without the caller's scale)
  float P;
};

// per-image variance from ldl_residual's partials, P = var^(1/5); with_dP: the P term's coefficient from ldl_map's
// partials.  Fixed-order sums over the whole workgroup: every thread calls it and gets the same values.
__device__ ImageStats image_stats(const Args &a, int b, bool with_dP, double2 *sh) {
  const int HW = a.H * a.W;
  double s1 = 0.0, s2 = 0.0;
  for (int j = threadIdx.x; j < a.nb1; j += NT) {
    const double2 v = a.p1[(size_t)b * a.nb1 + j];
    s1 += v.x;
    s2 += v.y;
  }
  const double2 s = block_sum2(s1, s2, sh);
  const double n = (double)HW;
  const double var = fmax((s.y - s.x * s.x / n) / (n - 1.0), 0.0);
  const float var_f = (float)var;
  ImageStats st;
  st.mean = (double)fabsf(a.rsrc[(size_t)b * HW]) + s.x / n;
  st.P = powf(var_f, 0.2f);
  st.pc = 0.0;
  if (with_dP) {
    double d = 0.0;
    for (int t = threadIdx.x; t < a.ntile; t += NT) d += a.p2[(size_t)b * a.ntile + t].y;
    const double dP = block_sum2(d, 0.0, sh).x;
    st.pc = dP * 0.2 * pow((double)var_f, -0.8) * 2.0 / (n - 1.0);   // var = 0: 0 * inf = NaN, as the reference
  }
  return st;
}

// ---------------------------------------------------------------------------------------------------- residuals ---
__global__ __launch_bounds__(NT) void ldl_residual(Args a) {
  __shared__ double2 sh[NT / 64];
  const int b = blockIdx.y, HW = a.H * a.W;
  const size_t img = (size_t)b * a.C * HW;
  const float r0 = resid(a.o, a.g, img, a.C, HW);
  double s1 = 0.0, s2 = 0.0;
  for (int u = 0; u < RES_PX; ++u) {
    const int i = blockIdx.x * (NT * RES_PX) + u * NT + threadIdx.x;
    if (i >= HW) break;
    const float r = resid(a.o, a.g, img + i, a.C, HW);
    const bool masked = a.e && r < resid(a.e, a.g, img + i, a.C, HW);
    a.rs[(size_t)b * HW + i] = masked ? -r : r;
    const double x = (double)r - (double)r0;
    s1 += x;
    s2 += x * x;
  }
  const double2 s = block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) a.p1[(size_t)b * a.nb1 + blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------------------- map ---
template <int KT, int MODE>
__global__ __launch_bounds__(NT) void ldl_map(Args a) {
  __shared__ float sr[LH][LW];
  __shared__ double2 sh[NT / 64];
  const int K = KT ? KT : a.k, R = K / 2;
  const int b = blockIdx.y, HW = a.H * a.W;
  const int tx0 = (blockIdx.x % a.tiles_x) * TW, ty0 = (blockIdx.x / a.tiles_x) * TH;
  const float *rs = a.rsrc + (size_t)b * HW;
  load_halo_tile(sr, ty0, tx0, R, a.H, a.W, [&](int at) { return MODE == LOCALVAR ? rs[at] : fabsf(rs[at]); });
  __syncthreads();
  const float P = MODE == LOCALVAR ? 1.f : image_stats(a, b, false, sh).P;   // (its block sums end in a barrier)
  const float inv_n = 1.f / (float)(K * K), inv_n1 = 1.f / (float)(K * K - 1);
  const bool want_g = MODE == LOSS || a.up;
  const int lx = threadIdx.x & (TW - 1);
  double lsum = 0.0, dP = 0.0;
  for (int h = 0; h < 2; ++h) {
    const int ly = (threadIdx.x / TW) + h * (TH / 2);
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= a.H || x >= a.W) continue;
    float s = 0.f;
    for (int dy = 0; dy < K; ++dy)
      for (int dx = 0; dx < K; ++dx) s += sr[ly + dy][lx + dx];
    const float mu = s * inv_n;
    float q = 0.f;
    for (int dy = 0; dy < K; ++dy)
      for (int dx = 0; dx < K; ++dx) {
        const float d = sr[ly + dy][lx + dx] - mu;
        q += d * d;
      }
    const float V = q * inv_n1;
    const size_t p = (size_t)b * HW + (size_t)y * a.W + x;
    float wv, av = 0.f;
    if (MODE == LOCALVAR) {
      wv = V;
      if (a.up) av = a.up[p];
    } else {
      const bool masked = signbit(a.rsrc[p]);
      wv = masked ? 0.f : P * V;
      if (MODE == LOSS) {
        const size_t at = (size_t)b * a.C * HW + (size_t)y * a.W + x;
        for (int c = 0; c < a.C; ++c) {
          const float ov = a.o[at + (size_t)c * HW], gv = a.g[at + (size_t)c * HW];
          const float d = wv * ov - wv * gv;
          lsum += (double)fabsf(d);
          av += sgnf(d) * (ov - gv);
        }
        if (masked) av = 0.f;
      } else if (a.up && !masked) {
        av = a.up[p];
      }
    }
    if (a.w) a.w[p] = wv;
    if (want_g) {
      const float Gv = av * P;
      a.G[p] = Gv;
      a.GM[p] = Gv * mu;
      dP += (double)av * (double)V;
    }
  }
  if (MODE != LOCALVAR && want_g) {
    const double2 t = block_sum2(lsum, dP, sh);
    if (threadIdx.x == 0) a.p2[(size_t)b * a.ntile + blockIdx.x] = t;
  }
}

// --------------------------------------------------------------------------------------------- backward gather ---
template <int KT, int MODE>
__global__ __launch_bounds__(NT) void ldl_grad(Args a) {
  __shared__ float sG[LH][LW], sGM[LH][LW];
  __shared__ float hG[LH][TW], hGM[LH][TW];
  __shared__ double2 sh[NT / 64];
  const int K = KT ? KT : a.k, R = K / 2;
  const int b = blockIdx.y, HW = a.H * a.W;
  const int tx0 = (blockIdx.x % a.tiles_x) * TW, ty0 = (blockIdx.x / a.tiles_x) * TH;
  const int lw = TW + 2 * R, lh = TH + 2 * R;
  for (int i = threadIdx.x; i < lh * lw; i += NT) {
    const int ly = i / lw, lx = i - ly * lw;
    const int y = ty0 - R + ly, x = tx0 - R + lx;
    float gv = 0.f, gm = 0.f;
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
      const size_t p = (size_t)b * HW + (size_t)y * a.W + x;
      gv = a.G[p];
      gm = a.GM[p];
    }
    sG[ly][lx] = gv;
    sGM[ly][lx] = gm;
  }
  double mean = 0.0, pc = 0.0;
  if (MODE != LOCALVAR) {
    const ImageStats st = image_stats(a, b, true, sh);
    mean = st.mean;
    pc = st.pc;
  }
  if (MODE == LOSS && a.loss && blockIdx.x == 0 && b == 0) {
    double l = 0.0;
    for (int i = threadIdx.x; i < a.B * a.ntile; i += NT) l += a.p2[i].x;
    l = block_sum2(l, 0.0, sh).x;
    if (threadIdx.x == 0) a.loss[0] = (float)(a.loss_scale * l);
  }
  __syncthreads();
  if (!a.grad) return;
  // row pass: hG[ly][lx] = sum over source columns px of mult(qx, px) G(py, px), for the tile's columns qx
  for (int i = threadIdx.x; i < lh * TW; i += NT) {
    const int ly = i / TW, lx = i - ly * TW;
    const int qx = tx0 + lx;
    float sg = 0.f, sgm = 0.f;
    if (qx < a.W) {
      for (int dx = 0; dx < K; ++dx) {
        const int px = qx - R + dx;
        if (px < 0 || px >= a.W) continue;
        const float m = (float)mult(qx, px, a.W, R);
        sg += m * sG[ly][lx + dx];
        sgm += m * sGM[ly][lx + dx];
      }
    }
    hG[ly][lx] = sg;
    hGM[ly][lx] = sgm;
  }
  __syncthreads();
  const float two_n1 = 2.f / (float)(K * K - 1);
  const int lx = threadIdx.x & (TW - 1);
  for (int h = 0; h < 2; ++h) {
    const int ly = (threadIdx.x / TW) + h * (TH / 2);
    const int qy = ty0 + ly, qx = tx0 + lx;
    if (qy >= a.H || qx >= a.W) continue;
    float tg = 0.f, tgm = 0.f;
    for (int dy = 0; dy < K; ++dy) {
      const int py = qy - R + dy;
      if (py < 0 || py >= a.H) continue;
      const float m = (float)mult(qy, py, a.H, R);
      tg += m * hG[ly + dy][lx];
      tgm += m * hGM[ly + dy][lx];
    }
    const size_t p = (size_t)b * HW + (size_t)qy * a.W + qx;
    const float rq = MODE == LOCALVAR ? a.rsrc[p] : fabsf(a.rsrc[p]);
    float gr = two_n1 * (rq * tg - tgm);
    if (MODE == LOCALVAR) {
      a.grad[p] = gr;
      continue;
    }
    gr += (float)(pc * ((double)rq - mean));
    const size_t at = (size_t)b * a.C * HW + (size_t)qy * a.W + qx;
    const float wv = MODE == LOSS ? a.w[p] : 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float ov = a.o[at + (size_t)c * HW], gv = a.g[at + (size_t)c * HW];
      float t = sgnf(ov - gv) * gr;
      if (MODE == LOSS) t += sgnf(wv * ov - wv * gv) * wv;
      a.grad[at + (size_t)c * HW] = a.scale * t;
    }
  }
}

// --------------------------------------------------------------------------------------------------------- host ---
struct Layout {
  size_t rs, w, G, GM, p1, p2, total;
  int nb1, tiles_x, ntile;
};

inline Layout layout(int B, int H, int W) {
  Layout L;
  const size_t n = (size_t)B * H * W;
  L.nb1 = (H * W + NT * RES_PX - 1) / (NT * RES_PX);
  L.tiles_x = (W + TW - 1) / TW;
  L.ntile = L.tiles_x * ((H + TH - 1) / TH);
  Carver c;
  L.rs = c.take(4 * n);
  L.w = c.take(4 * n);
  L.G = c.take(4 * n);
  L.GM = c.take(4 * n);
  L.p1 = c.take(sizeof(double2) * (size_t)B * L.nb1);
  L.p2 = c.take(sizeof(double2) * (size_t)B * L.ntile);
  L.total = c.end;
  return L;
}

// argument checks shared by every entry point, in the order the header documents
inline int check(int B, int C, int H, int W, int k, const void *ws, size_t ws_bytes) {
  if (k < 3 || k % 2 == 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0) return SSG_E_BADARG;
  if (k > KMAX) return SSG_E_TOOLARGE;
  if (H <= k / 2 || W <= k / 2) return SSG_E_IMAGESMALL;
  return check_workspace(ws, ws_bytes, layout(B, H, W).total);
}

inline Args make_args(const float *o, const float *g, const float *e, int B, int C, int H, int W, int k, void *ws,
                      const Layout &L) {
  Args a{};
  char *base = (char *)ws;
  a.o = o;
  a.g = g;
  a.e = e;
  a.rs = (float *)(base + L.rs);
  a.rsrc = a.rs;
  a.G = (float *)(base + L.G);
  a.GM = (float *)(base + L.GM);
  a.p1 = (double2 *)(base + L.p1);
  a.B = B;
  a.C = C;
  a.H = H;
  a.W = W;
  a.k = k;
  a.nb1 = L.nb1;
  a.tiles_x = L.tiles_x;
  a.ntile = L.ntile;
  a.scale = 1.f;
  return a;
}

template <int MODE>
void launch_map_grad(const Args &a, bool map, bool grad, hipStream_t st) {
  const dim3 grid((unsigned)a.ntile, (unsigned)a.B);
  if (a.k == 7) {
    if (map) hipLaunchKernelGGL((ldl_map<7, MODE>), grid, dim3(NT), 0, st, a);
    if (grad) hipLaunchKernelGGL((ldl_grad<7, MODE>), a.grad ? grid : dim3(1, 1), dim3(NT), 0, st, a);
  } else {
    if (map) hipLaunchKernelGGL((ldl_map<0, MODE>), grid, dim3(NT), 0, st, a);
    if (grad) hipLaunchKernelGGL((ldl_grad<0, MODE>), a.grad ? grid : dim3(1, 1), dim3(NT), 0, st, a);
  }
}

inline void launch_residual(const Args &a, hipStream_t st) {
  hipLaunchKernelGGL(ldl_residual, dim3((unsigned)a.nb1, (unsigned)a.B), dim3(NT), 0, st, a);
}

}  // namespace ldl
}  // namespace ssg

using namespace ssg::ldl;

extern "C" {

size_t ssg_ldl_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return layout(B, H, W).total;
}

int ssg_artifact_map(const float *output, const float *gt, const float *ema, int B, int C, int H, int W, int k,
                     float *w_out, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!output || !gt || !w_out || !workspace) return SSG_E_BADARG;
  const int rc = check(B, C, H, W, k, workspace, workspace_bytes);
  if (rc) return rc;
  const Layout L = layout(B, H, W);
  Args a = make_args(output, gt, ema, B, C, H, W, k, workspace, L);
  a.w = w_out;
  const hipStream_t st = (hipStream_t)stream;
  launch_residual(a, st);
  launch_map_grad<MAP>(a, true, false, st);
  return (int)hipGetLastError();
}

int ssg_artifact_map_backward(const float *output, const float *gt, const float *ema, const float *grad_w, int B, int C,
                              int H, int W, int k, float *grad_output, void *workspace, size_t workspace_bytes,
                              ssg_stream_t stream) {
  if (!output || !gt || !grad_w || !grad_output || !workspace) return SSG_E_BADARG;
  const int rc = check(B, C, H, W, k, workspace, workspace_bytes);
  if (rc) return rc;
  const Layout L = layout(B, H, W);
  Args a = make_args(output, gt, ema, B, C, H, W, k, workspace, L);
  a.up = grad_w;
  a.p2 = (double2 *)((char *)workspace + L.p2);
  a.grad = grad_output;
  const hipStream_t st = (hipStream_t)stream;
  launch_residual(a, st);
  launch_map_grad<MAP>(a, true, true, st);
  return (int)hipGetLastError();
}

int ssg_ldl_loss(const float *output, const float *gt, const float *ema, int B, int C, int H, int W, int k,
                 float loss_weight, int mean, float *loss_out, float *grad_output, void *workspace,
                 size_t workspace_bytes, ssg_stream_t stream) {
  if (!output || !gt || !loss_out || !workspace) return SSG_E_BADARG;
  const int rc = check(B, C, H, W, k, workspace, workspace_bytes);
  if (rc) return rc;
  const Layout L = layout(B, H, W);
  Args a = make_args(output, gt, ema, B, C, H, W, k, workspace, L);
  const double N = (double)B * C * H * W;
  a.w = (float *)((char *)workspace + L.w);
  a.p2 = (double2 *)((char *)workspace + L.p2);
  a.grad = grad_output;
  a.loss = loss_out;
  a.loss_scale = mean ? (double)loss_weight / N : (double)loss_weight;
  a.scale = (float)a.loss_scale;
  const hipStream_t st = (hipStream_t)stream;
  launch_residual(a, st);
  launch_map_grad<LOSS>(a, true, true, st);
  return (int)hipGetLastError();
}

int ssg_local_variance(const float *residual, int B, int H, int W, int k, float *v_out, const float *grad_v,
                       float *grad_residual, void *workspace, size_t workspace_bytes, ssg_stream_t stream) {
  if (!residual || !workspace || (!v_out && !grad_residual) || (!grad_v != !grad_residual)) return SSG_E_BADARG;
  const int rc = check(B, 1, H, W, k, workspace, workspace_bytes);
  if (rc) return rc;
  const Layout L = layout(B, H, W);
  Args a = make_args(nullptr, nullptr, nullptr, B, 1, H, W, k, workspace, L);
  a.rsrc = residual;
  a.w = v_out;
  a.up = grad_v;
  a.grad = grad_residual;
  const hipStream_t st = (hipStream_t)stream;
  launch_map_grad<LOCALVAR>(a, true, grad_residual != nullptr, st);
  return (int)hipGetLastError();
}

}  // extern "C"
