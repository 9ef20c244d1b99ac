// rgc_api_frontend.hip -- host side of the A1-A8 front end (rgc_frontend*): ScanRegistration::laserCloudHandler on the device
// (src/scanRegistration.cpp:89-730).  The kernels are in rgc_frontend.hip.
#include "rgc_ctx.h"

using namespace rgcapi;

extern "C" {

void rgc_default_fe_params(rgc_fe_params* p) {
  if (!p) return;
  p->n_scans = 16; p->min_range = 0.5; p->max_range = 80.0; p->use_intensity = 1;  // launch/run.launch:6,12-13,18
}

static int frontend_impl(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, const rgc_fe_params* prm, rgc_fe_out* out, int on_device, bool allow_spec = true) {
  if (!c || !xyzi || !prm || !out || n < 0 || n > (1 << 27)) return RGC_ERR_INVALID;
  if (n > (1 << 24)) return fail(c, RGC_ERR_INVALID, "sweep has %d points, the front-end's limit is 2^24", n);  // 32-bit sizes and candidate lists below
  if (!stride4_ok(stride_bytes)) return fail(c, RGC_ERR_INVALID, "front-end needs x,y,z,intensity: stride_bytes >= 16");
  const int NS = prm->n_scans;
  if (NS != 16 && NS != 32 && NS != 64) return fail(c, RGC_ERR_INVALID, "only 16, 32 or 64 scan lines (scanRegistration.cpp:69-72)");
  out->n_cloud = out->n_sharp = out->n_sharp_own = out->n_flat = out->n_inten = out->n_ground = 0;
  out->ground_valid = 0;
  c->fe.n_cloud = 0;
  memset(out->ring_count, 0, sizeof(out->ring_count));
  if (n == 0) return RGC_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int stride_f = stride_bytes / 4;
  const float* d_in;
  int rc = stage_in(c, xyzi, n, stride_bytes, on_device, &d_in);
  if (rc) return rc;
  const int nb = rgck::fe_blocks(n);
  const int nu = NS * 6, fcap = nu * 41;
  constexpr size_t kTailFlags = 304, kTailSt = 336, kTailFeat = 496;  // see OUTD below
  const size_t n4 = (size_t)4 * n;
  const size_t sizes[kFeBufs] = {n4, n4, (size_t)4 * 64 * nb, 4u * 132, 4u * 8, 4 * n4, n4, n4, n4, n4, n4, n4, n4, n4,
                            n4, n4, n4, n4, n4, n4, n4, n4, n4, (size_t)8 * 11 * nb, kTailFeat + 60u * (size_t)fcap,
                            4u * (size_t)nu * rgck::fe_slot_ints(), 4u * 8, 64u, 64u, 64u, 16u * 10 * (size_t)n, 4u * ((size_t)n / 2048 + 4), n4, n4};
  // OUTD is the sweep's "tail": ground sums / fit / distance sums (doubles 0..33), the flags, the filter's start-end state and the three
  // feature clouds in ONE buffer laid out like the pinned staging area behind the meta block, so that everything the host needs at the
  // end of the sweep comes down in ONE copy and the two small blocks are initialised by ONE
  for (int b = 0; b < kFeBufs; b++) if ((rc = ensure(c, c->fe.buf[b], sizes[b] + 64))) return rc;
#define FE(i, T) (c->fe.buf[FE_##i].as<T>())
  unsigned char* const tail = c->fe.buf[FE_OUTD].as<unsigned char>();
  int* const d_flags = (int*)(tail + kTailFlags);
  int* const d_st = (int*)(tail + kTailSt);
  float* const d_sharp = (float*)(tail + kTailFeat);
  float* const d_flat = d_sharp + 5 * (size_t)fcap;
  float* const d_inten = d_flat + 5 * (size_t)fcap;
  const int init16[16] = {0, 0, 0, 0, 0, 0, 0, 0, INT_MAX, -1, INT_MAX, 0, 0, 0, 0, 0};  // flags (zero) + the filter's state
  static_assert(sizeof(init16) == sizeof(rgck::SmallWords::fe), "the front-end's staged words");
  memcpy(c->h_small->fe, init16, sizeof(init16));
  HIPCHK(c, hipMemcpyAsync(d_flags, c->h_small->fe, sizeof(init16), hipMemcpyHostToDevice, s));
  rgck::FeParams fp{NS, prm->min_range, prm->max_range};
  rgck::fe_filter(s, d_in, stride_f, n, fp, FE(RING, int), d_st, FE(RANK, int), FE(HIST, int));
  rgck::fe_half(s, d_in, stride_f, n, FE(RING, int), d_st);
  rgck::fe_bucket(s, d_in, stride_f, n, NS, FE(RING, int), FE(RANK, int), FE(HIST, int), FE(META, int), d_st, FE(CL, float4), FE(INUM2, int),
                  FE(PICK, int), FE(IPICK, int), FE(LAB, int), FE(ILAB, int));
  // pinned staging: [0, 1024) meta + ground sums + flags, then the three feature clouds
  const size_t stage_need = 1024 + 3 * 20u * (size_t)fcap;
  if ((rc = ensure_pinned(c, c->fe.stage, stage_need, stage_need))) return rc;
  int* meta = (int*)c->fe.stage.p;                       // 129 ints
  int* fl = (int*)(c->fe.stage.p + 832);                 // 8 ints ([528, 800): the ground sums, fit and distance sums)
  unsigned char* h_feat = c->fe.stage.p + 1024;
  // The sweep's size after the range filter and its ring sizes are known on the device (k_fe_hist_scan); the host needs them only to
  // size launches and the selection kernel's LDS.  From the second sweep of a sequence on it does not wait for them: launches are sized
  // by the raw point count, the kernels read the size themselves (csp), the selection kernel's window by the largest ring of the
  // PREVIOUS sweep plus a quarter -- if a ring outgrows that (flag bit 1), the sweep is done again the slow way.
  const bool spec = allow_spec && c->fe.spec_on && c->fe.last_ns == NS && c->fe.last_max_ring > 0 && !out->cloud;
  int cs = n, max_ring = 0;
  const int* csp = nullptr;
  if (spec) {
    csp = FE(META, int) + 128;
    max_ring = std::min(n, c->fe.last_max_ring + c->fe.last_max_ring / 4 + 64);
  } else {
    HIPCHK(c, hipMemcpyAsync(meta, FE(META, int), sizeof(int) * 129, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    cs = meta[128];
    out->n_cloud = cs;
    for (int r = 0; r < NS; r++) { out->ring_count[r] = meta[r]; max_ring = std::max(max_ring, meta[r]); }
    if (cs == 0) return RGC_OK;
    if (out->cloud && out->cloud_cap < cs) return fail(c, RGC_ERR_INVALID, "cloud_cap %d < %d points", out->cloud_cap, cs);
  }
  rgck::fe_stencils(s, FE(CL, float4), cs, csp, FE(RANGE, float), FE(ANGLE, float), FE(INUM2, int), FE(INUM, int), FE(CURV, float), FE(CURV2, float),
                    FE(ICURV, float), FE(DSRC, float), FE(OSRC, float), FE(PICK, int));
  // A5: ground set (with multiplicities) -> weighted centroid / covariance -> plane (scanRegistration.cpp:308-431)
  rgck::fe_ground(s, FE(CL, float4), cs, csp, NS, FE(RANGE, float), FE(META, int), FE(GMARK, int), FE(MULT, int), FE(SCNT, int), FE(PART, double), FE(OUTD, double),
                  FE(OUTD, double) + 16);
  // OUTD: [0..10] the ground sums, [16..31] the plane fit, [32..33] the distance sums -- fitted on the device, read back with the features
  rgck::fe_ground_dist(s, FE(CL, float4), cs, csp, FE(MULT, int), FE(OUTD, double) + 16, FE(PART, double), FE(OUTD, double) + 32);
  // /laser_cloud_ground: pushes in reference order (with duplicates); empty when no ground seed was found
  // (only when the caller takes the list: the chained frame body does not, and these are four launches)
  if (out->ground_pts && out->ground_cap > 0) {
    rgck::exclusive_scan(s, FE(SCNT, int), FE(SPOS, int), cs, FE(BSUM, int));
    const int gcap_dev = 10 * n;
    rgck::fe_ground_list(s, FE(CL, float4), cs, csp, NS, FE(RANGE, float), FE(META, int), FE(SCNT, int), FE(SPOS, int), FE(GLIST, float4), gcap_dev);
  }
  // A7 + A8
  rgck::fe_select(s, FE(CL, float4), NS, FE(META, int), FE(CURV, float), FE(CURV2, float), FE(ICURV, float), FE(INUM, int), FE(GMARK, int),
                  FE(PICK, int), FE(IPICK, int), FE(LAB, int), FE(ILAB, int), FE(SLOTS, int), d_flags, max_ring, FE(SORTC, int), FE(SORTI, int));
  rgck::fe_emit(s, FE(CL, float4), NS, FE(SLOTS, int), FE(DSRC, float), FE(OSRC, float), d_sharp, d_flat, d_inten, fcap,
                d_flags + 4);
  // flags and the three feature clouds (at their capacity: ~80 kB each for 16 rings) come down together into pinned memory, one
  // synchronisation; the counts decide how much of each is handed to the caller
  double* gd = (double*)(c->fe.stage.p + 528);            // the tail's doubles 0..33 behind the 129 meta ints
  static_assert(528 + kTailFlags == 832 && 528 + kTailFeat == 1024, "the device tail mirrors the staging area from gd on");
  HIPCHK(c, hipMemcpyAsync(gd, tail, kTailFeat + 60u * (size_t)fcap, hipMemcpyDeviceToHost, s));
  if (spec) HIPCHK(c, hipMemcpyAsync(meta, FE(META, int), sizeof(int) * 129, hipMemcpyDeviceToHost, s));
  if (out->cloud) HIPCHK(c, hipMemcpyAsync(out->cloud, FE(CL, float4), sizeof(float) * 4 * (size_t)cs, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (spec) {
    if (fl[0] & 2) {  // a ring outgrew the window sized from the previous sweep (or really holds an oversize sector): the slow way decides
      c->fe.last_max_ring = 0;
      return frontend_impl(c, xyzi, n, stride_bytes, prm, out, on_device, false);
    }
    cs = meta[128];
    out->n_cloud = cs;
    max_ring = 0;
    for (int r = 0; r < NS; r++) { out->ring_count[r] = meta[r]; max_ring = std::max(max_ring, meta[r]); }
    if (cs == 0) return RGC_OK;
  }
  if (fl[0] & 2) return fail(c, RGC_ERR_INVALID, "a ring sector holds more than 2048 points");
  c->fe.n_cloud = cs;
  c->fe.last_ns = NS; c->fe.last_max_ring = max_ring;
  {  // ground message (:403-430) from the sums, the fit and the distance sums that just came down
    const long long gsize = (long long)(gd[10] + 0.5);
    if (gsize > 0) {
      const double* nrm = gd + 19;
      const double* V = gd + 22;
      const double* d2 = gd + 32;
      const double laderH = 0.56;  // :39
      double distance = d2[1] / d2[0], src1 = d2[0] / (double)gsize;  // :403-404
      if ((distance / laderH) > 1.1 || (distance / laderH) < 0.9) distance = laderH;  // :405-409
      if (src1 < 0.9) distance = 0.9 * laderH + 0.1 * distance;                       // :410-413
      double* g = out->groundparam;  // groundparam.msg order, :420-430
      g[0] = nrm[0]; g[1] = nrm[1]; g[2] = nrm[2];
      g[3] = V[1]; g[4] = V[4]; g[5] = V[7];
      g[6] = V[2]; g[7] = V[5]; g[8] = V[8];
      g[9] = distance; g[10] = 1 - src1;
      out->ground_valid = 1;
      out->n_ground = (int)gsize;
      if (out->ground_pts && out->ground_cap > 0) {
        const long long m = gsize < out->ground_cap ? gsize : out->ground_cap;
        HIPCHK(c, hipMemcpyAsync(out->ground_pts, FE(GLIST, float4), sizeof(float) * 4 * (size_t)m, hipMemcpyDeviceToHost, s));
      }
    }
  }
  const int ns = fl[4], nf = fl[5], ni = fl[6];
  out->n_sharp_own = ns; out->n_flat = nf; out->n_inten = ni;
  const bool add_inten = prm->use_intensity && ((double)ns / (double)nf < 0.3);  // :645-656
  out->n_sharp = ns + (add_inten ? ni : 0);
  if (out->feat_cap < out->n_sharp || out->feat_cap < nf || out->feat_cap < ni) return fail(c, RGC_ERR_INVALID, "feat_cap too small");
  if (ns) memcpy(out->sharp, h_feat, 20u * (size_t)ns);
  if (nf) memcpy(out->flat, h_feat + 20u * (size_t)fcap, 20u * (size_t)nf);
  if (ni) memcpy(out->inten, h_feat + 40u * (size_t)fcap, 20u * (size_t)ni);
  if (add_inten && ni) memcpy(out->sharp + 5 * (size_t)ns, h_feat + 40u * (size_t)fcap, 20u * (size_t)ni);
  const struct { void* dst; int src; } diag[7] = {{out->curvature, FE_CURV}, {out->curvature2, FE_CURV2}, {out->inten_curvature, FE_ICURV}, {out->label, FE_LAB},
                                                   {out->inten_label, FE_ILAB}, {out->picked, FE_PICK}, {out->ground_marked, FE_GMARK}};
  for (auto& d : diag) if (d.dst) HIPCHK(c, hipMemcpyAsync(d.dst, c->fe.buf[d.src].p, 4u * (size_t)cs, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
#undef FE
  return RGC_OK;
}

int rgc_frontend(rgc_ctx* c, const float* xyzi, int n, int stride_bytes, const rgc_fe_params* prm, rgc_fe_out* out) {
  return frontend_impl(c, xyzi, n, stride_bytes, prm, out, 0);
}
// the same with the sweep already on the device (e.g. rgc_pc2_unpack(..., out_on_device = 1)): no host copy of the input
int rgc_frontend_device(rgc_ctx* c, const float* d_xyzi, int n, int stride_bytes, const rgc_fe_params* prm, rgc_fe_out* out) {
  return frontend_impl(c, d_xyzi, n, stride_bytes, prm, out, 1);
}

int rgc_frontend_cloud_device(rgc_ctx* c, float** d_cloud, int* n) {
  if (!c || !d_cloud || !n) return RGC_ERR_INVALID;
  *d_cloud = c->fe.n_cloud > 0 ? c->fe.buf[FE_CL].as<float>() : nullptr;  // float4 {x, y, z, ring + 0.1 relTime}, ring-major
  *n = c->fe.n_cloud;
  return RGC_OK;
}

}  // extern "C"
