/*
 * rgc_hip.h -- C-ABI of librgc_hip.so: the MI355X (gfx950) scan-to-map registration path of RGC-SLAM.
 *
 * Plain C: opaque context, plain pointers and sizes, int status codes.  No C++/PCL/Eigen/ROS/torch types.
 * Every entry point names the reference interface it replaces; paths are relative to
 * /root/reference/rgc_slam/ (ROBOT-WSC/RGC-SLAM @2024_10_08).
 *
 * Ownership: the caller owns every host buffer for the duration of the call only (inputs are copied to
 *   the device before the call returns); the context owns all device memory, its HIP stream and events.
 * Threading: a context is NOT thread-safe and is bound to one HIP device; use one context per
 *   sequence / GPU, driven by one host thread (the reference drives registration from the single
 *   ICP_thread, src/RGC_odometer.cpp:408).  Every entry point that reaches the HIP runtime selects the context's
 *   device first (hipSetDevice) and leaves it current on return: a process may hold contexts on several GPUs and
 *   call each from a thread of its own, whatever device that thread had current (tests/test_abi.py audits it).
 * Errors: 0 = OK, negative = rgc_status; nothing aborts or throws across this boundary (the reference
 *   prints "lm not converged!!" and carries on, lsq_registration_impl.hpp:69-72; here that is the
 *   `lm_failed` output).  rgc_last_error() returns a human-readable message for the last failure.
 * There is NO CPU fallback: if no HIP device / kernel image is available every call fails with
 *   RGC_ERR_HIP.
 *
 * Matrices: 4x4 poses and 6x6 Hessians are ROW-MAJOR.  The 6-vector order is [rotation(3), translation(3)]
 *   with a LEFT-multiplied perturbation, exactly as LsqRegistration (lsq_registration_impl.hpp:139-143).
 */
#ifndef RGC_HIP_H
#define RGC_HIP_H

#include <stddef.h>

#if defined(__GNUC__) || defined(__clang__)
#define RGC_API __attribute__((visibility("default")))
#else
#define RGC_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rgc_ctx rgc_ctx;

typedef enum rgc_status {
  RGC_OK = 0,
  RGC_ERR_INVALID = -1,         /* bad argument / call order                                   */
  RGC_ERR_HIP = -2,             /* HIP runtime error (no device, OOM, launch failure, ...)     */
  RGC_ERR_TOO_FEW_POINTS = -3,  /* cloud has fewer than k_correspondences points (undefined in
                                   the reference, fast_gicp_impl.hpp:256-259)      */
  RGC_ERR_GRID_TOO_LARGE = -4,  /* bounding box / resolution needs more cells than max_cells   */
  RGC_ERR_NO_INPUT = -5,        /* source or target not set                                    */
  RGC_ERR_NONFINITE = -6,       /* input contains NaN/Inf coordinates                          */
  RGC_ERR_UNSUPPORTED = -7      /* the request has no meaning under the selected settings (e.g.
                                   unit normals asked for under a RegularizationMethod other
                                   than PLANE: rgc_set_regularization_method)                  */
} rgc_status;
/* What every entry point checks of its arguments before it touches anything (tests/fuzz/fuzz_null_args.py, fuzz_bad_args.py call each of them
 * with nothing, and with one bad argument at a time): a required pointer that is NULL, a negative count, a count above 2^27 points (2^24
 * for a PointCloud2 message), a stride that is not a multiple of 4 between the point type's minimum and 4096 bytes, a leaf size or a pose
 * that is not finite -- RGC_ERR_INVALID / RGC_ERR_NONFINITE, and the context is as it was.  What it cannot check and takes the caller's
 * word for: that a buffer holds as many points as the count says, and that a pointer called "device" (on_device != 0, the *_device
 * entries) is one -- unless RGC_CHECK_POINTERS=1 is in the environment when the context is created: then every such pointer is looked up first
 * (device memory of the context's GPU, an allocation with room for the count) and a host pointer or a short buffer is RGC_ERR_INVALID.
 * A HIP error is reported once, by the call it happened in (RGC_ERR_HIP, rgc_last_error); it does not surface again. */

/* enum order = fast_gicp::NeighborSearchMethod, include/fast_gicp/gicp/gicp_settings.hpp:8 */
typedef enum rgc_neighbor_method { RGC_DIRECT27 = 0, RGC_DIRECT7 = 1, RGC_DIRECT1 = 2, RGC_DIRECT_RADIUS = 3 } rgc_neighbor_method;

/* Parameter block = the setters the odometer calls on fast_gicp::FastVGICP (src/RGC_odometer.cpp:998-1006)
 * plus the constructor defaults they leave untouched.  Defaults: rgc_default_params(). */
typedef struct rgc_params {
  double voxel_res;             /* setResolution(1.0)            RGC_odometer.cpp:308,1000; fast_vgicp_impl.hpp:32-34 */
  int    max_iterations;        /* setMaximumIterations(25)      RGC_odometer.cpp:1001                                */
  int    lm_max_iterations;     /* lm_max_iterations_ = 10       lsq_registration_impl.hpp:17                          */
  double rotation_eps;          /* setRotationEpsilon (2e-3)     lsq_registration_impl.hpp:12,27-29                    */
  double translation_eps;       /* setTransformationEpsilon(1e-6) RGC_odometer.cpp:1003                               */
  double lm_init_lambda_factor; /* setInitialLambdaFactor (1e-9) lsq_registration_impl.hpp:18,32-34                    */
  int    k_correspondences;     /* setCorrespondenceRandomness (20) fast_gicp_impl.hpp:16,41-43; 2..32 supported       */
  int    neighbor_method;       /* setNeighborSearchMethod (RGC_DIRECT1) fast_vgicp_impl.hpp:23,37-39                  */
  long long max_cells;          /* cap on dense grid cells per cloud (default 1<<29)                                  */
} rgc_params;

RGC_API void rgc_default_params(rgc_params* p);

/* FastGICP::setRegularizationMethod (include/fast_gicp/gicp/fast_gicp.hpp:52, impl/fast_gicp_impl.hpp:46-48; enum order =
 * fast_gicp::RegularizationMethod, gicp_settings.hpp:6) and FastVGICP::setVoxelAccumulationMode (fast_vgicp.hpp:57,
 * impl/fast_vgicp_impl.hpp:41-43; enum order = VoxelAccumulationMode, gicp_settings.hpp:10).  The odometer calls neither
 * (src/RGC_odometer.cpp:998-1006 leaves PLANE, fast_gicp_impl.hpp:20, and ADDITIVE, fast_vgicp_impl.hpp:24).
 * Every value is implemented.  PLANE with ADDITIVE / ADDITIVE_WEIGHTED (one and the same AdditiveGaussianVoxel in the vendored FastVGICP,
 * fast_vgicp_voxel.hpp:137-141; the mode is looked at nowhere else) runs on the tuned kernels, which keep a point's covariance as the unit
 * normal of I - 0.999 n n^T (24 bytes).  NONE, MIN_EIG, NORMALIZED_MIN_EIG, FROBENIUS (fast_gicp_impl.hpp:262-293) and
 * VoxelAccumulationMode::MULTIPLICATIVE (fast_vgicp_voxel.hpp:76-99) run on a GENERAL route: a regularised 3x3 per point (48 bytes), every
 * point's exact k-NN through the cooperative search, a plain voxel pass, and the LM loop driven from the host over a linearisation that takes
 * the full source covariance -- the same entry points and the reference's arithmetic, about four times slower at c1 size (it is not the odometer's
 * path and has not been tuned).  On that route rgc_align_begin solves at once and rgc_align_end hands the result over; rgc_set_target_lazy and
 * rgc_set_knn_reuse have no effect; rgc_get_*_covariances returns no normals (RGC_ERR_UNSUPPORTED if asked); rgc_set_*_covariances takes any
 * symmetric 3x3.  RGC_ERR_UNSUPPORTED is otherwise unused by these calls; an out-of-range value is RGC_ERR_INVALID.
 * The reference computes covariances at align() under the method selected THEN (fast_gicp_impl.hpp:103-112); this library computes them when
 * a cloud is set, so changing the method (or additive <-> multiplicative) afterwards DROPS the clouds: set them again.  Select before setting. */
typedef enum rgc_regularization_method { RGC_REG_NONE = 0, RGC_REG_MIN_EIG = 1, RGC_REG_NORMALIZED_MIN_EIG = 2, RGC_REG_PLANE = 3, RGC_REG_FROBENIUS = 4 } rgc_regularization_method;
typedef enum rgc_voxel_accumulation_mode { RGC_VOXEL_ADDITIVE = 0, RGC_VOXEL_ADDITIVE_WEIGHTED = 1, RGC_VOXEL_MULTIPLICATIVE = 2 } rgc_voxel_accumulation_mode;
RGC_API int rgc_set_regularization_method(rgc_ctx* ctx, int method);
RGC_API int rgc_set_voxel_accumulation_mode(rgc_ctx* ctx, int mode);

/* FastVGICPCuda::setNearestNeighborSearchMethod / setKernelWidth (include/fast_gicp/gicp/fast_vgicp_cuda.hpp:21,58,61,
 * impl/fast_vgicp_cuda_impl.hpp:46-51,64-66,107-109,136-138): how a point's covariance is estimated.  RGC_COV_KNN (default; the reference's
 * CPU_PARALLEL_KDTREE and GPU_BRUTEFORCE): the moment of its k exact nearest neighbours.  RGC_COV_RBF (GPU_RBF_KERNEL,
 * src/fast_gicp/cuda/covariance_estimation_rbf.cu:59-151): the Gaussian-weighted moment of EVERY point of its cloud within max_dist.
 *   ball     B(i) = { j : key(i, j) <= max_dist_sq }, key = the fp32 ((dx*dx + dy*dy) + dz*dz) without FMA (the key of the exact kNN),
 *            max_dist_sq = (float)max_dist * (float)max_dist in fp32 (:70,75-78); the point itself is always a member
 *   moment   in fp64: w_j = exp(-(double)(float)kernel_width * (double)key) -- "kernel_width" is the exponent's FACTOR (:80,120) --,
 *            d_j = P_j - P_i, S0 = sum w_j, S1 = sum w_j d_j, S2 = sum w_j d_j d_j^T, m = S1 / S0, cov = S2 / S0 - m m^T
 *            (NormalDistribution::finalize, :46-52, with the origin at P_i: the same matrix without the reference's fp32 cancellation),
 *            summed over the ball in ascending position of the cloud's cell-sorted order, one chain per point: bit-reproducible
 *   then     the selected RegularizationMethod, as after the kNN moment (fast_vgicp_cuda.cu:210,218)
 * The reference pads the cloud to a multiple of 512 with points at the origin and does not mask them (:74,127-129): points within max_dist of
 * (0,0,0) gain phantom neighbours there.  That defect is not reproduced.
 * rgc_set_rbf_kernel: defaults 0.5, 3.0 (fast_vgicp_cuda_impl.hpp:31); max_dist <= 0 means 5 * kernel_width (:46-51) and is what the getter
 * returns; kernel_width must be finite and > 0 (as a float too), max_dist not NaN: otherwise RGC_ERR_INVALID and nothing changes.  It may be
 * called under either method; it takes effect under RGC_COV_RBF.
 * RGC_COV_RBF runs on the GENERAL route whatever the regularisation (a 3x3 per point, see above: the same entry points, the host-driven LM,
 * rgc_set_target_lazy / rgc_set_knn_reuse without effect).  k_correspondences plays no part and RGC_ERR_TOO_FEW_POINTS does not apply: a
 * cloud of one point is legal.  Changing the method, or the kernel while RBF is selected, DROPS the clouds (the rule of
 * rgc_set_regularization_method); setting the current value again drops nothing.  An out-of-range method is RGC_ERR_INVALID. */
typedef enum rgc_covariance_estimation { RGC_COV_KNN = 0, RGC_COV_RBF = 1 } rgc_covariance_estimation;
RGC_API int rgc_set_covariance_estimation(rgc_ctx* ctx, int method);
RGC_API int rgc_get_covariance_estimation(const rgc_ctx* ctx, int* method);
RGC_API int rgc_set_rbf_kernel(rgc_ctx* ctx, double kernel_width, double max_dist);
RGC_API int rgc_get_rbf_kernel(const rgc_ctx* ctx, double* kernel_width, double* max_dist);

/* FastVGICP construction / destruction (a stack local re-created per frame at RGC_odometer.cpp:998;
 * here the context is long-lived and re-used, device buffers grow on demand). */
RGC_API int  rgc_create(int hip_device, const rgc_params* params /* NULL = defaults */, rgc_ctx** out);
RGC_API void rgc_destroy(rgc_ctx* ctx);
/* setResolution / setCorrespondenceRandomness / setMaximumIterations ... in one struct.  A new voxel_res or k_correspondences prepares the
 * clouds the context holds again, from their inputs (a device cloud must still be where it was set from); refused with a solve in flight. */
RGC_API int  rgc_set_params(rgc_ctx* ctx, const rgc_params* params);
RGC_API int  rgc_get_params(const rgc_ctx* ctx, rgc_params* params);
/* FastVGICPCuda::setNeighborSearchMethod(method, radius) (include/fast_gicp/gicp/fast_vgicp_cuda.hpp:60, impl/fast_vgicp_cuda_impl.hpp:58-61,
 * src/fast_gicp/cuda/fast_vgicp_cuda.cu:42-95; NeighborSearchMethod::DIRECT_RADIUS, gicp_settings.hpp:8, "supported on only VGICP_CUDA").
 * RGC_DIRECT_RADIUS looks a source point up in every voxel whose integer offset (i, j, k) from the point's own cell lies in
 * [-ceil(r), ceil(r)]^3 with sqrt((double)(i*i + j*j + k*k)) <= r + 1e-3, in nested i, j, k order (fast_vgicp_cuda.cu:77-91): 1 offset below
 * r = 0.999, 7 from there, 19 from 1.4133, 27 from 1.7311, 33 at 2.0, 123 at 3.0, 485 at 4.9.  Every hit is a correspondence of its own with
 * the term of the other methods (src/fast_gicp/cuda/compute_derivatives.cu:50-92): w = sqrt(num_points), M = (C_B + R C_A R^T)^-1,
 * J = [skew(R a + t), -I].
 *   rgc_neighbor_offsets      the offset table of a method (0..2: the lists of fast_vgicp_voxel.hpp:10-44, in their order; 3: the rule above):
 *                             *n = the table's size, at most cap offsets (3 ints each) written to xyz (NULL: the size alone).  Host code, no
 *                             context, no GPU.  The table is also NDT's (rgc_ndt_set_params).  RGC_ERR_INVALID: NULL n, a method outside 0..3,
 *                             under method 3 a radius that is not finite and >= 0 or a table above RGC_NDT_MAX_OFFSETS (r >= 4.9...).
 *   rgc_set_neighbor_search   methods 0..2 ignore the radius, whatever it is (the reference's default argument is -1.0), and the stored one
 *                             stays; method 3 needs a finite radius >= 0 whose table has at most RGC_NDT_MAX_OFFSETS offsets: otherwise
 *                             RGC_ERR_INVALID and nothing changes.  (The reference builds an EMPTY table for a negative radius and solves over
 *                             nothing: not reproduced.)  Refused with a solve in flight, like rgc_set_params.  Drops no cloud; the
 *                             correspondences the last linearisation froze stay what rgc_compute_error evaluates (rgc_set_params' rule).
 *   rgc_get_neighbor_search   the selection and the stored radius (0.0 on a new context).
 * rgc_params keeps its layout: rgc_get_params reports neighbor_method == 3 while the radius method is selected, and while it is selected
 * rgc_set_params accepts 3 and keeps the stored radius, so get / modify / set round-trips (and an adaptor that pushes the whole block from every
 * setter keeps the selection).  The block carries no radius, so it cannot SELECT the method: 3 in rgc_set_params or rgc_create on a context
 * whose selection is another method is RGC_ERR_INVALID, as before -- rgc_set_neighbor_search selects it.
 * Under RGC_DIRECT_RADIUS rgc_linearize, rgc_compute_error, rgc_num_correspondences and rgc_align* run over a kernel of their own (a group of
 * lanes per source point, the table walked in strides) on both covariance routes, and the solve is ALWAYS driven by the host LM loop, whatever
 * RGC_LM_IMPL says: rgc_align_begin solves at once and rgc_align_end (and rgc_align_end_reframe through it) hands the result over, the rule of
 * the general route; rgc_set_target_lazy has no effect (a lazy target is completed before the solve: the full build's results).  Re-framed,
 * shared, borrowed, map-bound and swapped targets need nothing new.  The frozen list costs 52 bytes per source point and offset.
 * Results are bit-identical from run to run and between host and device inputs; fp64 after the fp32 points (the reference: fp32), a dense
 * grid (the reference's hash table gives up after max_bucket_scan_count probes: not reproduced), sums in a fixed order (the reference's
 * thrust reduction: unspecified). */
RGC_API int  rgc_neighbor_offsets(int method, double radius, int* xyz /* 3 * cap ints, nullable */, int cap, int* n);
RGC_API int  rgc_set_neighbor_search(rgc_ctx* ctx, int method, double radius);
RGC_API int  rgc_get_neighbor_search(const rgc_ctx* ctx, int* method, double* radius);
RGC_API const char* rgc_last_error(const rgc_ctx* ctx);
RGC_API const char* rgc_status_string(int status);
RGC_API const char* rgc_version(void);

/* setInputTarget (fast_vgicp_impl.hpp:56-63) / setInputSource (fast_gicp_impl.hpp:72-80).
 * xyz: first float of point 0; point i starts at (char*)xyz + i*stride_bytes (x,y,z consecutive floats;
 * stride 16 or 32 = pcl::PointXYZI padding welcome).  Setting a cloud drops its covariances (and, for the
 * target, the voxel map) exactly like the reference; the exact-kNN covariances (fast_gicp_impl.hpp:241-298),
 * and for the target the Gaussian voxel map (fast_vgicp_voxel.hpp:129-156), are computed on the device
 * (enqueued immediately on the context's stream).  n <= 2^27 points per cloud (RGC_ERR_INVALID beyond: the kernels
 * address the sorted 16-byte points with 32-bit byte offsets).
 * From its second cloud on a context re-uses the previous cloud's (widened) grid instead of measuring the bounding box first
 * -- the one host round trip of these calls; results are unaffected.  A cloud that does not fit is prepared again, transparently,
 * when the first call that consumes it finds out; by the same token RGC_ERR_NONFINITE / RGC_ERR_GRID_TOO_LARGE for such a cloud
 * may be returned by that consuming call (rgc_align, rgc_linearize, a getter ...) instead of by rgc_set_*.  RGC_SPEC_GRID=0 in
 * the environment restores the immediate check.
 * What is a function of the clouds alone, and what is not: the neighbour sets, the target's covariances and the voxel map are -- bit for bit, on
 * every route and on any context.  The SOURCE's kNN grid is steered by the scans the context has seen: its cell size follows how crowded the
 * previous scan's cells were (it starts at the voxel size, and rgc_set_params with another voxel_res puts it back there), and its box is the one
 * kept from the previous scans, widened, while the next scan fits it.  The four-lane search sums a point's moments in that grid's order, the box
 * decides which far-field points go to the cooperative kernel instead (rgc_stats::deferred_source), which sums them in another, and a
 * linearisation's sums run over the scan in the grid's order: THE LAST BITS OF THE SOURCE'S COVARIANCES -- and of cost, H, b and final_H -- MAY
 * DEPEND ON THE SCANS THE CONTEXT HAS SEEN BEFORE (measured: one ulp in 4 of 5729 rows behind another sweep).  They are identical from run to
 * run for the same sequence of calls, and between host and device inputs.  (tests/one_context_ops.py puts the cell size and the box back
 * before every registration it compares with a context of its own: route().) */
RGC_API int rgc_set_target(rgc_ctx* ctx, const float* xyz, int n, int stride_bytes);
RGC_API int rgc_set_source(rgc_ctx* ctx, const float* xyz, int n, int stride_bytes);
/* same, but xyz is DEVICE memory on the context's device (cloud already resident in HBM).
 * Streams: the target is prepared on rgc_stream(ctx); the SOURCE is prepared on a second, internal stream so that it overlaps the
 * (much larger) target's preparation, and rgc_align joins the two.  That internal stream is ordered after everything that was
 * enqueued on rgc_stream(ctx) before this frame's rgc_set_target* call (or before rgc_set_source* itself when no target preparation
 * is in flight): a source buffer written by rgc_upload, by the front-end or by the caller's own kernels on rgc_stream(ctx) is safe
 * to hand over without synchronising, provided those writes were enqueued before rgc_set_target*.  Writes enqueued between
 * rgc_set_target* and rgc_set_source_device must be complete (synchronised) first. */
RGC_API int rgc_set_target_device(rgc_ctx* ctx, const float* d_xyz, int n, int stride_bytes);
RGC_API int rgc_set_source_device(rgc_ctx* ctx, const float* d_xyz, int n, int stride_bytes);

/* LsqRegistration::linearize (lsq_registration.hpp:68; fast_vgicp_impl.hpp:119-180): rebuilds the voxel
 * correspondences and Mahalanobis matrices at T, returns cost and (if both non-NULL) H, b. */
RGC_API int rgc_linearize(rgc_ctx* ctx, const double T[16], double H[36], double b[6], double* cost);
/* LsqRegistration::compute_error (lsq_registration.hpp:69; fast_vgicp_impl.hpp:183-204): cost at T with the
 * correspondences and Mahalanobis matrices FROZEN at the last rgc_linearize. */
RGC_API int rgc_compute_error(rgc_ctx* ctx, const double T[16], double* cost);
RGC_API int rgc_num_correspondences(rgc_ctx* ctx, int* n_corr);

/* pcl::Registration::align(out, guess) -> LsqRegistration::computeTransformation
 * (lsq_registration_impl.hpp:53-79, LM step :125-172) + getFinalTransformation + getFinalHessian (:43-45)
 * + getFitnessScore (RGC_odometer.cpp:1009-1011).  Any output pointer may be NULL.
 *   final_T    : float 4x4 (final_transformation_ = x0.cast<float>(), :77)
 *   final_H    : 6x6 of the last accepted LM step (identity if none, :21,167)
 *   fitness    : mean squared 1-NN distance source->target (computed only if non-NULL)
 *   iterations : outer iterations executed;  converged: hasConverged();  lm_failed: "lm not converged!!" */
RGC_API int rgc_align(rgc_ctx* ctx, const float guess[16], float final_T[16], double final_H[36], double* fitness,
              int* iterations, int* converged, int* lm_failed);
/* rgc_align in two halves (rgc_align == begin + end).  rgc_align_begin enqueues the solve behind the clouds' preparation and
 * returns without waiting; rgc_align_end waits for it and returns what rgc_align returns.  Between the two the caller may do
 * anything that does not touch THIS context -- in particular prepare the next frame's clouds on a second context, so that
 * the preparation of frame i + 1 runs on the GPU while frame i is being solved (rgc_slam_amd.registration.PipelinedVGICP,
 * rgc::OdometryNode's replay).  want_fitness != 0 chains getFitnessScore behind the solve (rgc_align_end's `fitness` then costs
 * nothing extra).  Errors that a speculative grid defers (rgc_set_* above) may surface in rgc_align_end.
 * BETWEEN the two halves the context refuses (RGC_ERR_INVALID, "a solve is in flight") everything that would touch the solve's inputs:
 * new clouds, clearing or swapping them, another begin or a blocking rgc_align, the settings that re-route a cloud, the getters,
 * rgc_map_commit (but for the no-op commit of an unchanged map).  The same on the general covariance route, where rgc_align_begin runs the
 * solve at once and keeps its result for rgc_align_end.
 * Everything else RUNS with a solve in flight and leaves the solve's result what it would have been: the front-end, the leaf filter (whole and
 * in its two halves), rgc_uniform_sampling, rgc_deskew, rgc_transform_cloud, the PointCloud2 (un)packing, rgc_icp_align*, the rgc_mapreg_* calls,
 * rgc_map_reset / insert / evict / rebase of a map the solve's target is not bound to, and the blocks that say so themselves below (the keyframe
 * store, the pose graph, NDT); the search index and the features built on its walk (outlier filters, clustering, plane, normals, FPFH) are
 * refused, as their own blocks say.  tests/one_context_ops.py holds one column of this per operation. */
RGC_API int rgc_align_begin(rgc_ctx* ctx, const float guess[16], int want_fitness);
RGC_API int rgc_align_end(rgc_ctx* ctx, float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged,
                          int* lm_failed);
/* rgc_align_end on `solve`, then -- without going back to the caller -- the two steps a frame loop WITHOUT a fusion stage does with the
 * result: the world pose composed in fp64, world_T <- world_T * final_T (t_w_curr / q_w_curr, src/RGC_odometer.cpp:1201-1203), and the
 * next frame's target enqueued on `next` (the same context or the other one of a pair taking turns): the sub-map d_map re-expressed in
 * the new body frame, q = inverse rotation of world_T, t = -q * translation (:1250-1255), exactly rgc_set_target_reframed(next, d_map,
 * n, stride_bytes, q, t, d_scratch).  The host's turn-around between a frame's result and the next frame's first launch is on the
 * critical path of a dependent sequence; here it is a few microseconds of C instead of the caller's pose arithmetic and a second call.
 * world_T: 16 doubles, row-major 4x4, in: the world pose before this frame, out: after it.  Outputs as rgc_align_end.
 * On two contexts (next != solve) with the fitness chained to the solve, the next target is enqueued as soon as the solve's final POSE is
 * known -- the deciding launch posts it before it computes the score -- and the call then waits for the score: same results, the score's
 * ~25 us no longer in front of the next frame.
 * Failure is all or nothing for the caller's arguments: `next` (alive, no solve in flight), d_map / n / stride_bytes / d_scratch are
 * checked as rgc_set_target_reframed checks them BEFORE the solve is consumed -- such an error leaves the solve pending and world_T
 * untouched, and the call may be repeated with corrected arguments.  (A HIP or allocation failure inside the next target's preparation
 * is reported after the outputs and world_T have been written; rgc_last_error names the failing call.) */
RGC_API int rgc_align_end_reframe(rgc_ctx* solve, rgc_ctx* next, double world_T[16], const float* d_map, int n, int stride_bytes,
                                  float* d_scratch, float final_T[16], double final_H[36], double* fitness, int* iterations,
                                  int* converged, int* lm_failed);
/* ctx registers its scans to the target `owner` has prepared (rgc_set_target*, or rgc_map_commit: the resident local map), without
 * preparing or copying it: ctx's target becomes a non-owning alias of the owner's device buffers.  Two contexts can then take turns
 * on a sequence whose map does not change every frame (the next scan is prepared on one while the current one is solved on the
 * other).  The owner must stay alive and must not be destroyed while ctx uses the target; when the owner prepares a new target
 * (rgc_set_target*, a commit that rebuilds) ctx's next rgc_align* fails with RGC_ERR_INVALID until the target is shared again.
 * Synchronises both contexts.  No reference counterpart (the reference builds one FastVGICP per frame).
 * A borrowed target is the OWNER's, prepared under the owner's settings: rgc_set_params on ctx with another voxel_res or k (which prepares a
 * context's own clouds again) drops the alias -- share again once the owner holds a target under those settings; swapping, clearing or
 * setting covariances on a borrowed target is refused or drops it likewise. */
RGC_API int rgc_share_target(rgc_ctx* ctx, rgc_ctx* owner);
/* pcl::Registration::getFitnessScore() for an arbitrary pose */
RGC_API int rgc_fitness(rgc_ctx* ctx, const float T[16], double* fitness);
/* the `output` cloud of align(): pcl::transformPointCloud(*input_, output, final_transformation_)
 * (lsq_registration_impl.hpp:78) in the caller's point order; out stride in bytes (>= 12). */
RGC_API int rgc_get_aligned(rgc_ctx* ctx, const float T[16], float* out_xyz, int stride_bytes);
/* the same cloud left on the device: d_out_xyz is a device pointer (n_source * stride_bytes bytes); enqueued on the context's
 * stream, no synchronisation, no copy -- for callers that consume the aligned cloud on the GPU (the odometer's sub-map insert) */
RGC_API int rgc_get_aligned_device(rgc_ctx* ctx, const float T[16], float* d_out_xyz, int stride_bytes);

/* Lazy target.  Only the voxels the solve LOOKS UP enter its cost (update_correspondences, impl/fast_vgicp_impl.hpp:73-116: one voxel per
 * source point with DIRECT1), and a voxel's covariance needs the 20-NN covariances of that voxel's points only -- yet the reference builds
 * every covariance of the map every frame (setInputTarget, src/RGC_odometer.cpp:1007), and so does this library by default.  With
 * margin_cells > 0 a target set afterwards gets its grid at rgc_set_target* and the rest at rgc_align / rgc_align_begin, for the cells
 * within margin_cells voxels (Chebyshev) of a voxel the scan falls into at the guess: 8 % of the c-main map at a margin of 2.  Every
 * look-up of the solve is checked; one that lands on an occupied voxel outside the built part (the pose moved more than the margin
 * covers) makes rgc_align_end complete the map and solve again, and any other consumer of the target (getters, the fine seam,
 * rgc_share_target, a second solve on the same target) completes it first: results are those of the full build, bit for bit, always.
 * 0 (default): off.  rgc_stats::lazy_misses counts the solves that had to be repeated. */
RGC_API int rgc_set_target_lazy(rgc_ctx* ctx, int margin_cells);

/* Scheduling hint for two contexts taking turns on a dependent sequence -- every frame's target is the sub-map re-framed by the previous
 * pose (src/RGC_odometer.cpp:1248-1256), so only the NEXT scan can be prepared ahead: the next rgc_set_source* on ctx starts on the
 * GPU only when the target preparation other has enqueued last (rgc_set_target*) has finished, i.e. under other's solve instead of
 * beside its map's kNN launch.  Results are unaffected. */
RGC_API int rgc_hold_source_until_target_of(rgc_ctx* ctx, rgc_ctx* other);

/* getSourceCovariances / getTargetCovariances analogue (fast_gicp.hpp): PLANE-regularised 3x3 covariances
 * (row-major, n*9 doubles) and/or unit normals (n*3 doubles, sign arbitrary), caller point order. */
RGC_API int rgc_get_source_covariances(rgc_ctx* ctx, double* cov9 /* may be NULL */, double* normals /* may be NULL */);
RGC_API int rgc_get_target_covariances(rgc_ctx* ctx, double* cov9, double* normals);
/* FastGICP::setSourceCovariances / setTargetCovariances (include/fast_gicp/gicp/fast_gicp.hpp:58-61, impl/fast_gicp_impl.hpp:93-100):
 * n*9 doubles, row-major, caller point order, for the cloud set before.  Only covariances of the plane-regularised form
 * I - 0.999 n n^T (what this path and the reference's odometer produce, fast_gicp_impl.hpp:280-293) are representable here: any other
 * matrix is RGC_ERR_INVALID.  The target's voxel map is rebuilt from them. */
RGC_API int rgc_set_source_covariances(rgc_ctx* ctx, const double* cov9, int n);
RGC_API int rgc_set_target_covariances(rgc_ctx* ctx, const double* cov9, int n);
/* FastGICP::clearSource / clearTarget (fast_gicp.hpp:56-57, fast_gicp_impl.hpp:60-69) and FastVGICP::swapSourceAndTarget
 * (fast_vgicp_impl.hpp:46-53: the clouds change roles, the voxel map is rebuilt from the new target; covariances the caller set with
 * rgc_set_source/target_covariances travel with their cloud, like the reference's swap of source_covs_ / target_covs_ -- computed
 * ones are the same function of the cloud in either role). */
RGC_API int rgc_clear_source(rgc_ctx* ctx);
RGC_API int rgc_clear_target(rgc_ctx* ctx);
RGC_API int rgc_swap_source_and_target(rgc_ctx* ctx);
/* Gaussian voxel map dump (fast_vgicp_voxel.hpp:105-122): up to cap voxels, unordered.
 * coords 3*cap ints, num cap ints, mean 3*cap doubles, cov9 9*cap doubles; *count = total voxels. */
RGC_API int rgc_get_voxels(rgc_ctx* ctx, int cap, int* coords, int* num, double* mean, double* cov9, int* count);

/* ---- stages either side of the operator in the odometer's per-frame body (vg_ICP::ICP_thread) ----
 * on_device != 0: every cloud pointer of the call is device memory on the context's device. */
/* B2  vg_ICP::adjustDistortion (src/RGC_odometer.cpp:1441-1481), in place.  Points are x,y,z,intensity with
 * intensity = ring + 0.1 * relTime as the front-end encodes it (scanRegistration.cpp:207-210).
 * q_last_curr_xyzw / t_last_curr: the motion guess (IMU pre-integration or previous delta, :929,993-996).
 * on_device: returns once the kernel is enqueued on rgc_stream(ctx); later calls on this context, rgc_download and work the caller
 * enqueues on that stream see the de-skewed sweep (the frame body's next stage is the leaf filter, which reads it there). */
RGC_API int rgc_deskew(rgc_ctx* ctx, float* xyzi, int n, int stride_bytes, const double q_last_curr_xyzw[4],
                       const double t_last_curr[3], int on_device);
/* B3  pcl::VoxelGrid<PointXYZI>::filter with setLeafSize(leaf,leaf,leaf) (src/RGC_odometer.cpp:976-991).
 * out_xyzi: n*4 floats capacity (x,y,z,intensity centroids, 16-byte stride, ordered by leaf index); *n_out = leaves.
 * If the leaf grid would overflow int the input is returned unfiltered, like PCL.
 * (A context remembers the leaf box of the last cloud per leaf size and filters the next one on it without measuring its bounding
 * box first; the output does not depend on the box, and a cloud that leaves it is filtered again on its own.) */
RGC_API int rgc_voxelgrid(rgc_ctx* ctx, const float* xyzi, int n, int stride_bytes, float leaf, float* out_xyzi, int* n_out,
                          int on_device);
/* The same filter for a DEVICE cloud in two halves: begin enqueues it (on the leaf box kept from the previous cloud of this leaf size) and
 * returns, end waits and returns the point count -- repeating the filter when the kept box did not hold the cloud, so d_xyzi and d_out must
 * stay untouched in between.  The odometer's sub-map filter (src/RGC_odometer.cpp:985-991) depends only on the previous frame's pose: begun
 * when that frame ends and ended after the next sweep's own filter, it is off the frame's critical path.  Other rgc_voxelgrid calls may run
 * in between; one begin may be open per context. */
RGC_API int rgc_voxelgrid_begin(rgc_ctx* ctx, const float* d_xyzi, int n, int stride_bytes, float leaf, float* d_out);
RGC_API int rgc_voxelgrid_end(rgc_ctx* ctx, int* n_out);
/* What the last leaf filter on this context did: filled by every rgc_voxelgrid and rgc_voxelgrid_end (an rgc_voxelgrid_begin alone does not
 * change it), from the variables the filter itself used.  For tests and tuning: the filter's OUTPUT never depends on the route.
 * The filter sorts the points by counting them into buckets of the leaf grid (the leaves themselves for a dense cloud, whole grid rows
 * along x for a sweep, segments of 2^seg_shift leaves of a row for a large sparse cloud) and ranks them inside a bucket through one 64-bit
 * record per point, packed (13 bits of leaf x, the bucket's extent inside the record) or unpacked (32 bits of leaf x). */
#define RGC_VG_PATH_NONE 0       /* no filter has run on this context, or n == 0 */
#define RGC_VG_PATH_KEPT 1       /* filtered on the padded box kept from an earlier cloud of this leaf size: no bounding-box pass */
#define RGC_VG_PATH_MEASURED 2   /* the cloud's own leaf box was measured first */
#define RGC_VG_PATH_UNFILTERED 3 /* that box has more than INT_MAX leaves: output = input, like PCL */
typedef struct rgc_vg_route {
  int path;            /* RGC_VG_PATH_*: where the result (or the refusal) came from */
  int status;          /* what the call returned (RGC_OK, RGC_ERR_NONFINITE, RGC_ERR_GRID_TOO_LARGE, ...) */
  int repeated;        /* 1: a chain ran on the kept box first, a point lay outside it (bit 1 of kept_flags), and the filter ran again */
  int kept_box;        /* the box kept for this leaf size when the call began: 0 none, 1 used, 2 valid but its padded grid is neither
                        * sparse nor within max_cells (not used), 3 invalidated by an earlier call */
  int kept_flags;      /* flags word of the chain on the kept box (0 when there was none): 1 non-finite point, 2 point outside the box,
                        * 4 point within half the padding of a face */
  int box_invalidated; /* 1: this call dropped the kept box (kept_flags & 6): the next cloud of this leaf size is measured */
  int chain;           /* 1: the fields below describe the chain that produced the output; 0: no chain did (unfiltered copy, refusal) */
  int leaf_buckets;    /* 1: the sort's buckets are the leaves (dense cloud); 0: rows, or segments of rows */
  int seg_shift;       /* 0 leaves, 3..30 segments of 2^seg_shift leaves, 31 whole rows */
  int nseg;            /* buckets per grid row */
  int packed;          /* 1: packed records, 0: unpacked */
  int edge;            /* > 0: a kept box, points within `edge` leaves of its faces set flag 4 */
  int flags;           /* flags word of that chain */
  int minb[3], div[3]; /* the leaf grid used: a measured box also when chain == 0 and path != RGC_VG_PATH_NONE */
  int n, n_out;
} rgc_vg_route;
RGC_API int rgc_voxelgrid_route(rgc_ctx* ctx, rgc_vg_route* out);
/* pcl::UniformSampling<PointT>::filter with setRadiusSearch(leaf) (src/RGC_mapping.cpp:1533-1536, 2497-2500): one INPUT point per occupied leaf, the
 * one nearest the leaf's centre.  The argument rules, the meaning of on_device, the routes and the refusals are rgc_voxelgrid's (RGC_ERR_NONFINITE,
 * RGC_ERR_GRID_TOO_LARGE, RGC_ERR_INVALID for a bad stride or leaf; n = 0 gives *n_out = 0); it is that filter's chain with another last launch, and
 * rgc_voxelgrid_route reports it.  out_xyzc: n * 4 floats capacity; out_index (nullable): n ints, host or device like the clouds.
 *   Semantics, restated from PCL's filters/impl/uniform_sampling.hpp FROM MEMORY [3P-memory] (PCL is not available to this project; SURVEY A.6
 * says the same of VoxelGrid):
 *   - the leaf grid is the leaf filter's: inv = 1.0f / leaf, ijk = floor(fp32(p * inv)), the same min_b, div and idx = i + j dx + k dx dy;
 *   - a leaf's centre is c_a = fp32(fp32((float)ijk_a + 0.5f) * leaf) from the GLOBAL ijk; a point's key is d2 = (dx*dx + dy*dy) + dz*dz in fp32,
 *     not contracted; the winner has the smallest (d2, input index) -- PCL walks the input in order and replaces on strict < only, the same rule;
 *   - PCL's distance runs over the point's 4-float map; its fourth component adds the same constant to both sides of a comparison: ignored;
 *   - the winner's 16 bytes go out unchanged, {x, y, z, c} (c = 0 for a 12-byte input, as in the leaf filter), its input index to out_index.
 *   Defined here, unspecified in PCL: the leaves come in ASCENDING idx, the leaf filter's order (PCL walks an unordered_map).
 *   A grid of more than INT_MAX leaves follows THIS LIBRARY's rule for rgc_voxelgrid: RGC_VG_PATH_UNFILTERED, output = input (bit for bit),
 *   out_index = the identity.  What PCL's UniformSampling returns there is not known to this project. */
RGC_API int rgc_uniform_sampling(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, float leaf, float* out_xyzc, int* out_index /* nullable */,
                                 int* n_out, int on_device);
/* B9  vg_ICP::transformPointCloud(cloud, q, t) (src/RGC_odometer.cpp:1495-1514): q * p + t in fp64, stored fp32,
 * intensity copied; out_xyzi: n*4 floats.  on_device: both pointers are device memory and the call returns once the kernel is enqueued
 * on rgc_stream(ctx), like rgc_deskew. */
RGC_API int rgc_transform_cloud(rgc_ctx* ctx, const float* xyzi, int n, int stride_bytes, const double q_xyzw[4], const double t[3],
                                float* out_xyzi, int on_device);

/* B9 + setInputTarget in one call, for a sub-map that lives on the device (src/RGC_odometer.cpp:1248-1256 then :998-1007): d_xyzi (n
 * points, fixed between calls) re-expressed by q * p + t into d_scratch (n*4 floats, device) and prepared as the registration's target
 * -- grid, exact-kNN covariances, voxel map, like rgc_set_target_device -- without a host round trip: the re-framed cloud's bounding
 * box is derived from the input's (measured on the first call with a given d_xyzi, n) and the transform.  What a dependent sequence
 * does every frame with the pose the previous frame returned.
 * Seeds (round 5): while consecutive calls name the same (d_xyzi, n), the map's exact 20-NN search (fast_gicp_impl.hpp:241-298) starts
 * from what the last search of each point found -- its k-th neighbour distance, kept per ORIGINAL point (4 bytes each) and widened by the
 * fp32 rounding of the coordinates in two frames: only candidates under that bound are looked at, no running top-k is kept.  The result
 * does NOT depend on what the seeds hold: a search that does not find exactly its k neighbours under the bound (a buffer rewritten in
 * place, a different cloud at the same address) is repeated without it, so "fixed between calls" is what makes the call fast, not what
 * makes it right.  Covariances are bit-identical with and without seeds (RGC_KNN_SEEDS=0 in the environment switches them off).
 * Neighbour lists (round 5): on top of the seeds the library keeps, per point, the 20 neighbours its last exact search found and its OWN
 * COPY of the map (112 bytes per point in all).  Every call compares d_xyzi with that copy, bit for bit, in the pass that re-frames it;
 * when nothing differs (and |q|^2 is within 1e-9 of 1: any quaternion normalised in fp64), a point whose list carries a certificate -- the gap behind its 20th
 * neighbour is wider than the fp32 rounding of the coordinates in any two frames can bridge -- takes its neighbours from the list instead
 * of searching (about 99 % of a map; rgc_stats::searched_target counts the rest); one differing coordinate and the call searches every
 * point again and rebuilds the lists.  The result is the search's, bit for bit, either way (RGC_KNN_CACHE=0 switches the lists off).
 * A lazy target (rgc_set_target_lazy) keeps seeds but no lists.
 * WHEN THIS HELPS, AND WHEN IT CANNOT: seeds and lists belong to point IDENTITIES.  They serve a caller that keeps its sub-map in the world
 * frame on the device and hands the same points over every frame -- i.e. one that has dropped the reference's per-frame body-frame leaf filter
 * (pcl::VoxelGrid over the re-framed sub-map, src/RGC_odometer.cpp:985-991: its centroids are a new point set every frame) and filters once
 * per keyframe instead (rgc_map_commit does).  A caller that keeps the reference's frame body (rgc::OdometryNode does) never hits them: its
 * target is a map the library has not seen, every frame, and costs the full search.  rgc_set_knn_reuse(ctx, RGC_REUSE_NONE) gives exactly
 * that cost for any map, and is what bench.py's `value` is timed with.
 * Preconditions: d_scratch must not overlap d_xyzi (RGC_ERR_INVALID: the input is read while the output is written, and a buffer has
 * one bounding-box hint); a d_scratch that is 16-byte aligned (anything hipMalloc / rgc_device_alloc returns) takes the fused path
 * -- re-framing inside the preparation's counting pass -- any other 4-byte aligned address the re-framing runs as its own launch.
 * A pose that is none -- a non-finite q or t (the NaN a diverged solve hands on through rgc_align_end_reframe), a zero quaternion -- is refused
 * with RGC_ERR_NONFINITE before anything is touched. */
RGC_API int rgc_set_target_reframed(rgc_ctx* ctx, const float* d_xyzi, int n, int stride_bytes, const double q_xyzw[4], const double t[3],
                                    float* d_scratch);
/* What a context keeps between the targets rgc_set_target_reframed prepares (no reference counterpart: the reference keeps nothing, it
 * builds a FastVGICP per frame, src/RGC_odometer.cpp:998).  Results never depend on the mode, bit for bit.
 *   RGC_REUSE_NONE   nothing: every target is searched like a map the library has not seen (no per-point state, no copy of the map)
 *   RGC_REUSE_SEEDS  the k-th distances of the last search (4 bytes per point)
 *   RGC_REUSE_LISTS  seeds + neighbour lists + the library's copy of the map (112 bytes per point; the default).  If the device cannot hold
 *                    them the context drops to RGC_REUSE_SEEDS by itself and carries on (rgc_get_knn_reuse tells).
 * Takes effect with the next rgc_set_target_reframed; lowering the mode frees the buffers it no longer needs (synchronises the context).
 * RGC_KNN_SEEDS=0 / RGC_KNN_CACHE=0 in the environment set a context's INITIAL mode to NONE / SEEDS (rgc_create). */
typedef enum rgc_knn_reuse { RGC_REUSE_NONE = 0, RGC_REUSE_SEEDS = 1, RGC_REUSE_LISTS = 2 } rgc_knn_reuse;
RGC_API int rgc_set_knn_reuse(rgc_ctx* ctx, int mode);
RGC_API int rgc_get_knn_reuse(const rgc_ctx* ctx, int* mode);

/* ---- A1-A8  ScanRegistration::laserCloudHandler (src/scanRegistration.cpp:89-730): range/NaN filter, ring + rel-time
 * assignment, curvature stencils, ground marking + weighted-PCA ground plane, occlusion mask, per-ring 6-sector
 * selection of sharp / flat / intensity features.  Input: the raw sensor cloud x,y,z,intensity in firing order
 * (what pcl::fromROSMsg yields from /velodyne_points, :107-108).  All output buffers are caller-allocated HOST memory.
 * Outputs = the node's published topics (:689-727): cloud = /velodyne_cloud_2 (ring-major, intensity = ring +
 * 0.1*relTime), sharp = /laser_cloud_sharp, inten = /laser_cloud_inten, flat = /laser_cloud_flat (features are
 * x,y,z,intensity,normal_x with normal_x the weight of :501,554,609), ground_pts = /laser_cloud_ground,
 * groundparam = /ground_param (ground_msg/groundparam.msg field order).  Per-point diagnostics may be NULL. */
typedef struct rgc_fe_params {
  int    n_scans;        /* scan_line: 16 / 32 / 64 (:57,69)          */
  double min_range;      /* minimum_range 0.5 (:59)                    */
  double max_range;      /* maxmum_range 80 (launch/run.launch:13)     */
  int    use_intensity;  /* USE_intensity (:58,645)                    */
} rgc_fe_params;
typedef struct rgc_fe_out {
  float* cloud; int cloud_cap; int n_cloud;                 /* cloud_cap points * 4 floats (NULL: not downloaded) */
  float* sharp; float* flat; float* inten; int feat_cap;    /* feat_cap features * 5 floats each                  */
  int n_sharp, n_sharp_own, n_flat, n_inten;                /* n_sharp includes the appended intensity corners    */
  float* ground_pts; int ground_cap; int n_ground;          /* ground_cap * 4 floats (may be NULL); n_ground total */
  double groundparam[11]; int ground_valid;                 /* ground_valid = 0 <=> "groundsize0" (:354-357)      */
  int ring_count[64];
  float *curvature, *curvature2, *inten_curvature;          /* cloud_cap each, optional                           */
  int *label, *inten_label, *picked, *ground_marked;        /* cloud_cap each, optional                           */
} rgc_fe_out;
RGC_API void rgc_default_fe_params(rgc_fe_params* p);
RGC_API int rgc_frontend(rgc_ctx* ctx, const float* xyzi, int n, int stride_bytes, const rgc_fe_params* params, rgc_fe_out* out);
/* the same with the sweep already resident on the device (a pointer from rgc_device_alloc, e.g. filled by
 * rgc_pc2_unpack(..., out_on_device = 1)): the message bytes are the only thing that crosses PCIe */
RGC_API int rgc_frontend_device(rgc_ctx* ctx, const float* d_xyzi, int n, int stride_bytes, const rgc_fe_params* params, rgc_fe_out* out);
/* the ring-major cloud of the LAST front-end call where it lies on the device (n x {x, y, z, ring + 0.1 relTime}, 16-byte stride), so
 * that de-skew / VoxelGrid / setInputSource can follow without a PCIe round trip (pass out->cloud = NULL to skip its download).
 * The pointer belongs to the context and is valid until the next front-end call; rgc_deskew(..., on_device = 1) may modify it in place. */
RGC_API int rgc_frontend_cloud_device(rgc_ctx* ctx, float** d_cloud, int* n);

/* ---- scalar host stages of the frame body (no GPU needed; kept in the same library so the adaptor is complete) ----
 * Quaternions are x,y,z,w.  ground[11] = ground_msg/groundparam order: norm xyz, vector1 xyz, vector2 xyz, distance,
 * source (ground_msg/msg/groundparam.msg:2-12; ground_s, include/rgc_slam/utility.h:382-389). */
/* C9  result extraction (src/RGC_odometer.cpp:1011-1016): Matrix4f -> (q_last_curr_l, t_last_curr_l) */
RGC_API int rgc_extract_pose(const float T[16], double q_xyzw[4], double t[3]);
/* B1  gyro-only delta-q guess + mid-point delta-p/delta-v (src/RGC_odometer.cpp:883-931,1418-1438) */
RGC_API int rgc_imu_preintegrate(const double* stamps, const double* gyr3, const double* acc3 /* may be NULL */, int n,
                                 double prev_time, double cur_time, double dq_xyzw[4], double dq2_xyzw[4] /* NULL ok */,
                                 double dp[3] /* NULL ok */, double dv[3] /* NULL ok */);
/* B1  the IMU side of the odometer's callbacks: vg_ICP::imu_callback (src/RGC_odometer.cpp:444-486: the first 100 messages are
 * dropped, biases removed) and ComplementaryFilter (:545-625: median filters over 201 / 41 / 41 accelerometer samples --
 * Mid_Filter, include/rgc_slam/utility.h -- complementary roll / pitch, integrated yaw) -> IMU.Rwi, the attitude the frame body
 * initialises the pose from (:866-871) and blends pitch / roll towards (:1206-1214).  Plain host code, no GPU. */
typedef struct rgc_imu_filter {
  double ba[3], bg[3];          /* imu_s::ba / bg (utility.h:253-254), subtracted from every sample */
  int    dropped;               /* of the first 100 messages (:446-451) */
  int    count;                 /* IMU.count: samples accepted */
  double t_last;                /* imu_last.t */
  double roll, pitch, yaw;      /* rad */
  double roll_last, pitch_last; /* imu_last.roll / pitch */
  double Rwi[9];                /* IMU.Rwi, row-major */
  double mf_buf[3][201];        /* Mid_Filter::data_buf of accx_MF(201), accy_MF(41), accz_MF(41) (:39) */
  int    mf_count[3];
} rgc_imu_filter;
RGC_API void rgc_imu_filter_init(rgc_imu_filter* f);
/* one sensor_msgs/Imu message.  Returns 1 and the bias-free sample (what the callback pushes into accBuf / gyrBuf for
 * rgc_imu_preintegrate) when the message is accepted, 0 while the first 100 are being dropped, < 0 on error. */
RGC_API int rgc_imu_filter_push(rgc_imu_filter* f, double stamp, const double acc[3], const double gyr[3], double acc_out[3], double gyr_out[3]);

/* B7  the ground-change detector in front of the fusion (src/RGC_odometer.cpp:1034-1087): a plane mismatch while the IMU pitches
 * (>= 0.02 twice and |pitch of delta_q_imu| > 0.5 deg) switches the ground factor off for 25 frames, after which the new plane is
 * re-associated with a remembered one (pitch / roll within 4 deg) or remembered itself.  Plain host code. */
typedef struct rgc_ground_gate {
  int    gflag;                 /* :328 */
  int    changegroundflag;      /* :327, starts at 25 */
  double q_w_curr_delta[4];     /* :20, x y z w */
  int    n_history;
  double history[64][4];        /* histoary_pose (:298); the oldest entry is overwritten beyond 64 */
} rgc_ground_gate;
RGC_API void rgc_ground_gate_init(rgc_ground_gate* g);
RGC_API void rgc_ground_gate_remember(rgc_ground_gate* g);  /* histoary_pose.push_back(q_w_curr_delta) of the first sub-map frame (:969) */
/* one frame: returns the new gflag (the ground factor is used when USE_GROUND && gflag == 0, :1088) and q_w_curr_f (:1086-1087) */
RGC_API int rgc_ground_gate_step(rgc_ground_gate* g, const double ground_last[11], const double ground_cur[11], const double q_lidar_xyzw[4],
                                 const double t_lidar[3], const double dq_imu_xyzw[4] /* NULL: identity */, const double q_w_curr_xyzw[4],
                                 double q_w_curr_f_xyzw[4]);

/* B7  the pose-fusion problem the reference builds for Ceres (src/RGC_odometer.cpp:1025-1032,1088-1119,1188-1193;
 * factors src/lidarFactor.hpp:132-172,228-265,311-350) */
typedef struct rgc_fuse_in {
  double q_lidar_xyzw[4];    /* q_last_curr_l (:1016)                                              */
  double t_lidar[3];         /* t_last_curr_l (:1015)                                              */
  double fitness;            /* vgicp_source = getFitnessScore() (:1010)                           */
  int    use_ground;         /* USE_GROUND && gflag == 0 (:1088)                                   */
  double ground_last[11];    /* ground_last                                                        */
  double ground_cur[11];     /* ground_cur                                                         */
  double q_w_curr_f_xyzw[4]; /* q_w_curr_delta^-1 * q_w_curr, normalised (:1086-1087)              */
  double ground_cov;         /* 0.2 (:1092)                                                        */
  int    use_imu;            /* USE_IMU && imuflag == 1 (:1104)                                    */
  double q_imu_xyzw[4];      /* delta_q_imu; its weight follows :1107-1116                         */
  int    max_iterations;     /* 6 (:1190)                                                          */
} rgc_fuse_in;
RGC_API void rgc_default_fuse_in(rgc_fuse_in* in);
RGC_API int rgc_fuse_pose(const rgc_fuse_in* in, double q_xyzw[4], double t[3], int* iterations /* NULL ok */);
/* B8  pose composition + 0.95/0.05 pitch-roll blend in DEGREES (src/RGC_odometer.cpp:1194-1214);
 * R_imu_wl = IMU.Rwi * R_il, row-major, only read when use_imu */
RGC_API int rgc_compose_pose(const double q_w_curr[4], const double t_w_curr[3], const double q_fused[4], const double t_fused[3],
                             const double t_lidar[3], int use_imu, const double R_imu_wl[9], double q_w_out[4], double t_w_out[3],
                             double t_last_curr_out[3] /* NULL ok */);
/* Utility::R2ypr / ypr2R (include/rgc_slam/utility.h:105-147): degrees, Rz*Ry*Rx, row-major 3x3 */
RGC_API void rgc_R2ypr(const double R[9], double ypr_deg[3]);
RGC_API void rgc_ypr2R(const double ypr_deg[3], double R[9]);

/* per-align statistics (reported by bench.py) */
typedef struct rgc_stats {
  int n_source, n_target, n_voxels, n_corr;
  int outer_iterations, n_linearize, n_error;
  long long target_cells, source_cells;
  int deferred_target, deferred_source; /* queries handled by the cooperative kNN kernel */
  double source_crowding;               /* mean number of points in a scan point's own kNN-grid cell (sum count^2 / n) */
  int lazy_misses;                      /* lazy target: solves repeated on the completed map since the context was created */
  int searched_target;                  /* queries of the target's last preparation whose k neighbours were SEARCHED: n_target, or -- a map handed
                                         * over again by rgc_set_target_reframed, unchanged -- the few whose neighbour list carries no certificate */
  int lm_fallbacks;                     /* solves whose one-launch (resident) LM gave up and that were solved again by the chained launches (same
                                         * result) since the context was created: 0 unless the device was badly oversubscribed */
} rgc_stats;
RGC_API int rgc_get_stats(rgc_ctx* ctx, rgc_stats* out);

/* ---- device plumbing for callers that keep clouds resident in HBM (bench, ROS adaptor) ---- */
RGC_API int  rgc_device_alloc(rgc_ctx* ctx, size_t bytes, void** d_ptr);
RGC_API int  rgc_device_free(rgc_ctx* ctx, void* d_ptr);
/* Page-locked HOST memory (hipHostMalloc, visible to every device) for a caller's staging buffers: a copy between the device and
 * pageable memory is staged by the runtime in a blocking hop, and the first touch of fresh pageable pages costs milliseconds (the
 * host-staged node's one 8.8 ms frame in round 3); out of these buffers the copies of rgc_set_*, rgc_voxelgrid, rgc_frontend run at
 * PCIe rate.  No context needed; rgc_host_free(NULL) is a no-op. */
RGC_API int  rgc_host_alloc(size_t bytes, void** h_ptr);
RGC_API int  rgc_host_free(void* h_ptr);
RGC_API int  rgc_upload(rgc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);   /* async on ctx stream */
RGC_API int  rgc_download(rgc_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronous          */
RGC_API int  rgc_synchronize(rgc_ctx* ctx);
RGC_API void* rgc_stream(rgc_ctx* ctx); /* the context's main hipStream_t (everything except the source's preparation, see rgc_set_source_device) */

/* ---- f3: wire and disk formats at the edges of the path ----
 * sensor_msgs/PointCloud2 <-> device arrays without PCL: pcl::fromROSMsg (src/scanRegistration.cpp:107-108) and pcl::toROSMsg
 * (:689-727, src/RGC_odometer.cpp:1348).  Fields in the order x, y, z, intensity, ring, time; offset < 0 = the message has
 * no such field (-> 0, ring -> -1).  datatype = sensor_msgs/PointField constants (INT8 1 ... FLOAT32 7, FLOAT64 8).
 * strict != 0 reproduces fromROSMsg<PointXYZI>'s field matching: a field whose datatype is not FLOAT32 is NOT mapped (stays
 * 0); strict = 0 converts any numeric type. */
typedef struct rgc_pc2_layout {
  int point_step;
  int offset[6];
  int datatype[6];
  int is_bigendian;
  int strict;
} rgc_pc2_layout;
/* data: width*height points of point_step bytes (host).  xyzi_out: n x 4 floats (host, or device if out_on_device);
 * ring_out / time_out: n ints / floats, nullable (same residency). */
RGC_API int rgc_pc2_unpack(rgc_ctx* ctx, const void* data, int n_points, const rgc_pc2_layout* layout, float* xyzi_out, int* ring_out,
                           float* time_out, int out_on_device);
/* kind 0: PointXYZI message (point_step 32), in = n x 4 {x,y,z,intensity}; kind 1: PointXYZINormal message (point_step 48),
 * in = n x 5 {x,y,z,intensity,normal_x}.  data_out: n * point_step bytes (host). */
RGC_API int rgc_pc2_pack(rgc_ctx* ctx, int kind, const float* in, int n, int in_on_device, void* data_out);
typedef struct rgc_pc2_field { char name[16]; int offset; int datatype; int count; } rgc_pc2_field;
/* the PointField table pcl::toROSMsg emits for that point type; returns the number of fields (<= cap), *point_step set */
RGC_API int rgc_pc2_point_fields(int kind, rgc_pc2_field* out, int cap, int* point_step);
/* one line of the TUM trajectory file f_save_pose_evo (src/RGC_odometer.cpp:1315-1316): "stamp tx ty tz qx qy qz qw\n" with
 * std::fixed, 6 decimals for the stamp and 9 for the rest.  Returns the length written (excluding the NUL) or < 0. */
RGC_API int rgc_tum_line(double stamp, const double t[3], const double q_xyzw[4], char* buf, int cap);
/* key-frame cloud to a .pcd file (src/RGC_odometer.cpp:1353-1354 writes ASCII): binary = 0 -> DATA ascii like
 * pcl::io::savePCDFileASCII (precision 8), binary = 1 -> DATA binary, 16 bytes per point (FIELDS x y z intensity). */
RGC_API int rgc_pcd_write(const char* path, const float* xyzi, int n, int binary);

/* ---- f4: loop-closure ICP = pcl::IterativeClosestPoint<PointType2,PointType2> as configured and used at
 * src/RGC_mapping.cpp:2050-2069: setMaxCorrespondenceDistance, setMaximumIterations(100), setTransformationEpsilon(1e-6),
 * setEuclideanFitnessEpsilon(1e-6), setRANSACIterations(0); setInputSource(latestKeyFrameCloud), setInputTarget(
 * nearHistoryKeyFrameCloud), align() with the identity guess, hasConverged(), getFitnessScore(), getFinalTransformation(). */
typedef struct rgc_icp_params {
  int max_iterations;                 /* 100 */
  double max_correspondence_distance; /* poseGraphSearchRadius * 2 */
  double transformation_epsilon;      /* 1e-6: translation^2 <= eps and cos(angle) >= 1 - eps */
  double euclidean_fitness_epsilon;   /* 1e-6: relative change of the correspondence MSE */
} rgc_icp_params;
enum { RGC_ICP_NOT_CONVERGED = 0, RGC_ICP_ITERATIONS = 1, RGC_ICP_TRANSFORM = 2, RGC_ICP_ABS_MSE = 3, RGC_ICP_REL_MSE = 4,
       RGC_ICP_NO_CORRESPONDENCES = 5 };   /* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
typedef struct rgc_icp_result {
  int iterations, converged, state, n_correspondences;
  double fitness;                     /* getFitnessScore(): mean squared nearest-neighbour distance at the final transformation */
} rgc_icp_result;
RGC_API void rgc_default_icp_params(rgc_icp_params* p);
/* source / target: host AoS, x,y,z first, same stride.  final_T: row-major 4x4 float (getFinalTransformation()). */
RGC_API int rgc_icp_align(rgc_ctx* ctx, const float* source, int n_source, const float* target, int n_target, int stride_bytes,
                          const rgc_icp_params* params, float final_T[16], rgc_icp_result* result);

/* ---- f1: scan-to-map FEATURE registration of the mapping node, src/RGC_mapping.cpp:1069-1358 ----
 * Replaces, per mapping frame: kdtreeCornerFromMap/kdtreeSurfFromMap->setInputCloud (:1073-1074), the four association
 * loops (:1092-1282: pointAssociateToMap, 5-NN, PCA line test / QR plane fit) and ceres::Solve over para_q/para_t and
 * para_q_last/para_t_last with LidarEdgeFactor / LidarPlaneNormFactor under HuberLoss(0.1) (:1078-1341,
 * src/lidarFactor.hpp:9-51,91-121), twice (:1076).  The ground block (:1314-1340, Ground_DeltaFactor_goable) and the IMU
 * block (:1285-1312, RelativeRFactor + two PitchRollFactor) are optional inputs.
 * Features are n x 4 floats {x, y, z, weight} (PointXYZINormal's x,y,z,normal_x); quaternions are x,y,z,w. */
typedef struct rgc_mapreg_report {
  double initial_cost, final_cost;  /* ceres Summary: 1/2 sum rho(|r|^2) before / after the solve */
  int iterations, successful;       /* LM iterations run (<= 6) and accepted steps */
  int n_edge_cur, n_plane_cur, n_edge_last, n_plane_last; /* residual blocks: corner_num, surf_num, cornerLast_num, surfLast_num */
} rgc_mapreg_report;
/* one Ground_DeltaFactor_goable (src/lidarFactor.hpp:352-403) as created at RGC_mapping.cpp:1326-1337, NULL loss */
typedef struct rgc_mapreg_ground {
  double last_v1[3], last_v2[3], last_norm[3], last_distance; /* g_last: vector_1, vector_2, vector_norm, distance */
  double cur_norm[3], cur_distance;                          /* g_cur: vector_norm, distance */
  double q_history[4];                                       /* histoary_q = q_w_curr_f (x,y,z,w) */
  double last_q[4], last_t[3];                               /* last_q_q, last_t_t: the fixed previous pose */
  double p_var;                                              /* ground_cov (0.2) */
} rgc_mapreg_ground;
/* the IMU block of RGC_mapping.cpp:1285-1312 (USE_IMU == 1 && map_update != 0), NULL loss: RelativeRFactor::Create(delta_q_imu,
 * imu_cov) on (para_q_last, para_q) (src/lidarFactor.hpp:174-226) and PitchRollFactor::Create(pitch, roll, 0.02) on para_q and
 * on para_q_last (:434-468).  The caller computes imu_cov (0.004 / 0.4, :1288-1293) and the pitch / roll targets in radians
 * (ypr of IMUTemp.Rwi * R_il and of IMULast.Rwi * R_il, :1299-1310) as the reference does. */
typedef struct rgc_mapreg_imu {
  double delta_q[4];             /* delta_q_imu (x,y,z,w) */
  double imu_cov;                /* q_var of the RelativeRFactor */
  double pitch_cur, roll_cur;    /* pl_tmp, rl_tmp */
  double pitch_last, roll_last;  /* pl_last, rl_last */
  double pr_var;                 /* q_var of both PitchRollFactor (0.02) */
} rgc_mapreg_imu;
/* laserCloudCornerFromMapDS / laserCloudSurfFromMapDS (host AoS, x,y,z first; at least 5 points each) */
RGC_API int rgc_mapreg_set_maps(rgc_ctx* ctx, const float* corner_map, int n_corner, const float* surf_map, int n_surf, int stride_bytes);
/* association only (kind 0 = edge against the corner map, 1 = plane against the surf map): factors8 (nullable) receives
 * n x 8 doubles: edge {point_a[3], point_b[3], var, valid}, plane {norm[3], negative_OA_dot_norm, 0, 0, var, valid} */
RGC_API int rgc_mapreg_associate(rgc_ctx* ctx, int kind, const float* feat_xyzw, int n, const double q_xyzw[4], const double t[3],
                                 double* factors8, int* n_valid);
/* poses: q_w_curr[4] t_w_curr[3] q_w_last[4] t_w_last[3], in/out.  *gate_failed = 1 (poses untouched) when the size gate of
 * :1069 is not met.  report: one entry per pass of the two-pass loop (nullable).  ground_cur / ground_last (nullable): the
 * ground block on (para_q, para_t) resp. (para_q_last, para_t_last) -- pass them when the reference's condition at :1314 holds.
 * imu (nullable): the IMU block -- pass it when the condition at :1285 holds. */
RGC_API int rgc_mapreg_optimize(rgc_ctx* ctx, const float* corner_cur, int n_ccur, const float* surf_cur, int n_scur,
                                const float* corner_last, int n_clast, const float* surf_last, int n_slast,
                                const rgc_mapreg_ground* ground_cur, const rgc_mapreg_ground* ground_last,
                                const rgc_mapreg_imu* imu, double poses[14], rgc_mapreg_report report[2], int* gate_failed);
/* the normal equations one LM iteration of rgc_mapreg_optimize starts from, read out (the counterpart of rgc_linearize): the four
 * association loops at poses_assoc, then H (12 x 12 row-major, full and symmetric; rows 0-2 / 3-5 the rotation / translation of the
 * current pose on the local parameterisation, 6-11 the last pose's), g (12) and the robust cost of those frozen factors at
 * poses_eval (NULL: at poses_assoc).  n_factors: n_edge_cur, n_plane_cur, n_edge_last, n_plane_last.  factors8 (nullable, each entry
 * nullable): the factors of {corner_cur, surf_cur, corner_last, surf_last}, n x 8 doubles each in rgc_mapreg_associate's layout.
 * Needs rgc_mapreg_set_maps; does NOT apply the size gate of :1069, and any feature set may be empty. */
RGC_API int rgc_mapreg_linearize(rgc_ctx* ctx, const float* corner_cur, int n_ccur, const float* surf_cur, int n_scur,
                                 const float* corner_last, int n_clast, const float* surf_last, int n_slast,
                                 const rgc_mapreg_ground* ground_cur, const rgc_mapreg_ground* ground_last,
                                 const rgc_mapreg_imu* imu, const double poses_assoc[14], const double poses_eval[14],
                                 double H[144], double g[12], double* cost, int n_factors[4], double* const factors8[4]);


/* ---- f2: rolling local map resident on the device ----
 * The odometer keeps a deque of <= slipwide (3) keyframe clouds in the WORLD frame (src/RGC_odometer.cpp:1237-1247), and every
 * frame re-expresses all of them in the new body frame (:1248-1256), VoxelGrid-filters the concatenation (:985-991) and hands it
 * to a fresh FastVGICP (:998,1007): 3 kd-trees, N_t covariances and the voxel map are rebuilt per FRAME even when no keyframe
 * changed.  Here the keyframes stay in HBM in a map frame (world minus an origin that the caller keeps near the sensor so that
 * fp32 coordinates stay small), the registration runs in that frame (guess = T_w_curr * T_last_curr, result = the new world pose)
 * and the target (filter + grid + covariances + voxels) is rebuilt, on the device, only when a keyframe was inserted or evicted.
 * Numerics differ from the reference by the frame the 0.3 m leaf lattice and the 1 m voxel lattice are aligned to (map axes
 * instead of the previous body axes); the parity definition of this row: DESIGN.md section 6 (f2) and EXPERIMENTS.md "6e". */
typedef struct rgc_map_info {
  int n_keyframes;
  long long n_points;            /* world-frame points held (before the leaf filter) */
  int n_target;                  /* points of the committed target, -1 if the map changed since the last commit */
  unsigned long long revision;   /* bumped by every insert / evict / rebase / reset */
  int oldest_id, newest_id;      /* -1 when empty */
  double origin[3];
} rgc_map_info;
/* drops every keyframe; origin (nullable = 0,0,0): the world point the map frame is centred on */
RGC_API int rgc_map_reset(rgc_ctx* ctx, const double origin[3]);
/* surroundingCloud.push_back(transformPointCloud(cloud, q_w_curr, t_w_curr)) (:1237): q * p + (t - origin) in fp64, stored fp32,
 * intensity copied.  xyzi: x,y,z,intensity (stride >= 16), host or (on_device) device memory.  *keyframe_id (nullable): its id. */
RGC_API int rgc_map_insert(rgc_ctx* ctx, const float* xyzi, int n, int stride_bytes, const double q_w_xyzw[4], const double t_w[3],
                           int on_device, int* keyframe_id);
/* eviction: first every keyframe whose pose is farther than radius from center (skipped when center is NULL or radius <= 0), then
 * the oldest ones until at most max_keyframes remain (pop_front, :1242-1247; skipped when max_keyframes <= 0) */
RGC_API int rgc_map_evict(rgc_ctx* ctx, int max_keyframes, const double center[3], double radius, int* n_evicted);
/* moves the map frame's origin (every stored point shifts by old - new, fp64 -> fp32) */
RGC_API int rgc_map_rebase(rgc_ctx* ctx, const double new_origin[3]);
/* makes the map the registration target: pcl::VoxelGrid(leaf) over the keyframes in insertion order (:985-991) + setInputTarget
 * (:1007), all on the device.  A no-op when nothing changed since the last commit and the target is still bound (rgc_set_target*
 * unbinds it).  Poses passed to rgc_align / rgc_linearize are then map-frame poses (world translation minus origin).
 * With a solve in flight on the context anything but that no-op is refused before a byte is written (the filter's output buffer is the one
 * the bound target was set from); a commit that fails further down leaves the context WITHOUT a target rather than with one whose input
 * has been overwritten. */
RGC_API int rgc_map_commit(rgc_ctx* ctx, float leaf, int* n_target);
RGC_API int rgc_map_get_info(rgc_ctx* ctx, rgc_map_info* out);
/* which = 0: the stored keyframe points, 1: the committed target; up to cap points (x,y,z,intensity) to the host, *n = total */
RGC_API int rgc_map_download(rgc_ctx* ctx, int which, float* out_xyzi, int cap, int* n);

/* ---- f5: the mapping node's keyframe store resident on the device, with batched sub-map assembly ----
 * The mapping node keeps, per keyframe, a BODY-frame corner / surf / scan cloud (cornerCloudKeyFrames, surfCloudKeyFrames,
 * scanCloudKeyFrames) and a 6-DoF key pose (cloudKeyPoses6D) that the pose graph keeps correcting (correctKeyFramePoseGraph,
 * src/RGC_mapping.cpp:1618-1686), and assembles the clouds it registers against from them in three places: the surrounding maps of f1
 * (extractSurroundingKeyFramesAndMap, :1503-1616), the source and target of f4 (detectLoopClosure, :2180-2216) and the global map
 * (publishGlobalMap, :2508-2537).  Each is: for every selected keyframe transformPointCloud(cloud, &pose6D) (:2567-2612), concatenated
 * in selection order, then a pcl::VoxelGrid.  Here the keyframes stay in HBM in their body frames, the poses are mutable, and ONE launch
 * transforms any selection under the CURRENT poses; rgc_mapreg_set_maps_device / rgc_icp_align_device consume the result where it lies.
 * (The odometer's rgc_map_* store above holds world-frame points and cannot move a keyframe.)
 *   Points: a keyframe's clouds are stored as 16-byte points {x, y, z, c} in the body frame; c is whatever the caller keeps in the fourth
 * float (intensity for scans, normal_x for features: both are copied by :2585,2608-2609).  Input stride >= 16, host or device memory
 * (on_device: every cloud pointer of the call); a kind may be empty (n = 0, pointer NULL).  Ids are the caller's (cloudKeyPoses3D's
 * intensity, :1876,1584); pushing an id twice is RGC_ERR_INVALID.  Storage grows geometrically, earlier keyframes keep their content; a kind
 * holds at most 2^27 points.  A host cloud is on the device when rgc_kf_push returns, a device cloud is read in stream order on
 * rgc_stream(ctx).
 *   Poses: rgc_kf_pose = PointXYZIRPYT's x, y, z, roll, pitch, yaw (include/rgc_slam/utility.h:284-293), radians.  The rotation is computed
 * on the HOST in fp64 by the reference's chain (:2575-2576): float roll / pitch / yaw -> * rad2deg (180.0 / M_PI, :197) -> Utility::ypr2R
 * in degrees (utility.h:123-147: rgc_ypr2R) -> Eigen quaternion; the device then applies q * p + t with rgc_transform_cloud's
 * arithmetic (:2581), so that assembling ONE keyframe equals rgc_transform_cloud with that quaternion bit for bit.  A non-finite pose is
 * RGC_ERR_NONFINITE at rgc_kf_push / rgc_kf_set_poses, and the store is as it was.
 *   rgc_kf_assemble: for each id IN THE ORDER GIVEN (an id may repeat), for each kind in kind_mask (bit k = kind k) in ASCENDING kind
 * order, the keyframe's points in stored order.  {CORNER} and {SURF} separately give the surrounding maps (:1584-1602), {CORNER, SURF}
 * the loop clouds (:2186-2191, 2209-2214) and the global map (:2516-2521), {SCAN} the global scan map (:2526).  *n_raw = points before
 * the filter.  leaf > 0: the concatenation goes through the library's leaf filter on the device (rgc_voxelgrid: same output, same
 * refusals, rgc_voxelgrid_route tells); leaf <= 0: the concatenation itself.  *n_out points {x, y, z, c} are written to out_xyzc (host,
 * or 16-byte aligned device memory if on_device; stream-ordered then, like rgc_transform_cloud).  cap (points) too small -- below n_raw
 * without a filter, below n_out with one -- is RGC_ERR_INVALID with *n_raw / *n_out still reported, nothing written: size the buffer and
 * call again (cap = 0 with out_xyzc NULL asks for the counts).  An id that is not in the store, kind_mask outside 1..7, a selection
 * of more than 2^27 points: RGC_ERR_INVALID, nothing written.  n_ids = 0 is an empty cloud.
 *   ALWAYS the current poses: the reference caches the transformed surrounding clouds by id (:1551-1595) and so keeps a stale transform
 * for a keyframe that stays in the neighbourhood across a pose-graph correction; that quirk is NOT reproduced.
 *   State machine: the rgc_kf_* calls touch the store, staging of their own, the leaf filter's scratch and the caller's output -- never a
 * cloud or a solve of the registration.  With a solve in flight (rgc_align_begin .. rgc_align_end) every one of them RUNS, and the solve's
 * result is what it would have been (rgc_kf_assemble waits for the context's stream like rgc_voxelgrid does). */
enum { RGC_KF_CORNER = 0, RGC_KF_SURF = 1, RGC_KF_SCAN = 2, RGC_KF_KINDS = 3 };
typedef struct rgc_kf_pose { float x, y, z, roll, pitch, yaw; } rgc_kf_pose;
typedef struct rgc_kf_info {
  int n_keyframes;
  long long n_points[3];         /* body-frame points held, per kind */
  unsigned long long revision;   /* bumped by every push / set_poses / reset that changed the store */
} rgc_kf_info;
/* drops every keyframe (the buffers are kept) */
RGC_API int rgc_kf_reset(rgc_ctx* ctx);
/* cornerCloudKeyFrames / surfCloudKeyFrames / scanCloudKeyFrames [keyFrameNum] = ... and cloudKeyPoses6D->push_back (src/RGC_mapping.cpp:1909-1924) */
RGC_API int rgc_kf_push(rgc_ctx* ctx, int id, const rgc_kf_pose* pose, const float* corner, int n_corner, const float* surf, int n_surf,
                        const float* scan, int n_scan, int stride_bytes, int on_device);
/* correctKeyFramePoseGraph (src/RGC_mapping.cpp:1618-1686): new poses for n keyframes; all or nothing (an unknown id, a non-finite pose: no
 * pose changes).  n = 0 is a no-op. */
RGC_API int rgc_kf_set_poses(rgc_ctx* ctx, const int* ids, const rgc_kf_pose* poses, int n);
RGC_API int rgc_kf_get_info(rgc_ctx* ctx, rgc_kf_info* out);
RGC_API int rgc_kf_assemble(rgc_ctx* ctx, const int* ids, int n_ids, unsigned kind_mask, float leaf, float* out_xyzc, int cap, int on_device,
                            int* n_raw, int* n_out);
/* ---- which keyframes to assemble: the mapping node's three selections and what they rest on ----
 * Travelled distance and angle (src/RGC_mapping.cpp:1887-1908): computed on the host by rgc_kf_push in fp32 and never recomputed (the reference does
 * not either).  The first keyframe of a store has 0; then travel[p] = travel[p-1] + sqrtf((dx*dx + dy*dy) + dz*dz) with the differences against the
 * pose stored AT THAT MOMENT for the previous position (cloudKeyPoses6D->back(), corrected or not), and travel_angle[p] = travel_angle[p-1] +
 * fabsf(rad_delta), rad_delta = yaw - last.yaw as a float wrapped once by -+ 2 M_PI in double (:1903-1905).  rgc_kf_get_travel: either output nullable;
 * an unknown id is RGC_ERR_INVALID, nothing written.
 *   The radius gate of all three selections [3P-memory: pcl::KdTreeFLANN::radiusSearch over flann::L2_Simple<float>]:
 * r2 = (float)((double)radius * (double)radius); a key pose is inside when d2 = (dx*dx + dy*dy) + dz*dz (fp32, not contracted) < r2.  STRICT: a pose
 * exactly on the radius is outside.  The tests pin this rule; it is NOT pinned against FLANN itself, which is not available to this project.
 *   The key positions are mirrored on the device as float4 {x, y, z, position} (with the travelled distances and ids beside them), uploaded again
 * only when the store's revision has moved (push, rgc_kf_set_poses, an applied rgc_pgo_optimize, reset).  One gate launch computes d2 and the
 * predicate; no kd-tree is built.  Results are bit-identical from run to run.
 *   rgc_kf_select_surrounding (extractSurroundingKeyFramesAndMap, :1525-1548; radius 15, density 0.3 there): the key positions inside the gate
 * around `center`, in ascending store position, through rgc_uniform_sampling at leaf `density`; out_ids = the winners' ids in ascending leaf
 * index, *n_in_radius = poses inside the gate.  DEVIATION: the reference hands PCL the radius result in ascending DISTANCE, so on an exact tie of two
 * poses' distances to a leaf centre its winner is the one nearer the query; here it is the one at the lower store position.  Only exact ties differ.
 * (The reference's cache of transformed clouds, :1551-1595, is not reproduced: see rgc_kf_assemble.)
 *   rgc_kf_select_global (publishGlobalMap, :2493-2505; density 0.5 there): the same over every key position.
 *   rgc_kf_detect_loop (detectLoopClosure, :2141-2225).  L = the last store position.  R = history_search_radius + (travel[L] - distance_by_loop) *
 * drift_factor in fp32 (:2148).  The gate uses r2 from R, so a negative R searches |R| while the threshold below uses the signed value, as the
 * reference's text does.  A pose qualifies when it is inside the gate around pose L, fabsf(travel[p] - travel[L]) > loop_keyframe_dis_diff + R (fp32
 * add) and id >= min_key_id.  The candidate is the qualifying pose with the smallest (d2, position): the reference's "first in sorted order that
 * passes, skipping ids < 10" (:2159-2172) is this minimum -- DEVIATION only where FLANN orders two poses of EQUAL d2 otherwise.  None qualifying, or
 * closest_id == latest_id: found = 0.  History (:2195-2216): for i = -history_search_num .. +history_search_num the position p_closest + i,
 * skipped when < 0 or >= L, or when its id is < 0 or >= latest_id; the rest in that order to history_ids.  No corner or surf point among them (the
 * reference's empty nearHistoryKeyFrameCloud): found = 0.  The candidate reports latest / closest ids and poses as stored now (closest_id = -1
 * when nothing qualified), the signed search radius and the number of poses inside the gate.
 *   Common: cap too small is RGC_ERR_INVALID with the counts reported and nothing written (rgc_kf_assemble's convention); an empty store gives empty
 * results and found = 0; a non-finite argument, radius <= 0 or density <= 0 is RGC_ERR_INVALID; the leaf filter's refusals pass through
 * (rgc_voxelgrid_route tells the route of the sampling).  State machine as the other rgc_kf_* calls: they run with a solve in flight. */
typedef struct rgc_kf_loop_params {
  float history_search_radius;   /* historyKeyframeSearchRadius = 5, :155 */
  float drift_factor;            /* DRIFT_FACTOR = 0.02, :159 */
  float distance_by_loop;        /* DistanceByLoop = 0: the caller's state, :158, 2130-2135 */
  float loop_keyframe_dis_diff;  /* loopKeyframeDisDiff = 20, :160 */
  int history_search_num;        /* historyKeyframeSearchNum = 50, :157 */
  int min_key_id;                /* 10, :2166 */
} rgc_kf_loop_params;
typedef struct rgc_kf_loop_candidate {
  int found;
  int latest_id, closest_id;
  rgc_kf_pose latest_pose, closest_pose;
  float search_radius;
  int n_in_radius;
} rgc_kf_loop_candidate;
RGC_API int rgc_kf_get_travel(rgc_ctx* ctx, const int* ids, int n, float* distance /* nullable */, float* angle /* nullable */);
RGC_API int rgc_kf_select_surrounding(rgc_ctx* ctx, const float center[3], float radius, float density, int* out_ids, int cap, int* n_in_radius,
                                      int* n_out);
RGC_API int rgc_kf_select_global(rgc_ctx* ctx, float pose_density, int* out_ids, int cap, int* n_out);
RGC_API void rgc_default_kf_loop_params(rgc_kf_loop_params* p);
RGC_API int rgc_kf_detect_loop(rgc_ctx* ctx, const rgc_kf_loop_params* params, rgc_kf_loop_candidate* out, int* history_ids, int cap, int* n_history);
/* rgc_mapreg_set_maps for maps that lie on the context's device (what rgc_kf_assemble(..., on_device = 1) wrote): the same checks, the same
 * grids, bit for bit, minus the upload.  The buffers are read in stream order on rgc_stream(ctx) and not kept. */
RGC_API int rgc_mapreg_set_maps_device(rgc_ctx* ctx, const float* d_corner, int n_corner, const float* d_surf, int n_surf, int stride_bytes);
/* rgc_icp_align for a source and a target on the context's device: the same checks, the same result, bit for bit, minus the uploads */
RGC_API int rgc_icp_align_device(rgc_ctx* ctx, const float* d_source, int n_source, const float* d_target, int n_target, int stride_bytes,
                                 const rgc_icp_params* params, float final_T[16], rgc_icp_result* result);

/* ---- 4-DoF pose-graph optimisation over the keyframe store's key poses: PoseGraphOptimize4DoF (src/RGC_mapping.cpp:2303-2466) with
 * FourDOFError / AngleLocalParameterization (src/lidarFactor.hpp:490-595), the link between f4's drift matrix and f5's poses ----
 * For the selected keyframes IN THE CALLER'S ORDER (positions 0 .. N-1: copy_cloudKeyPoses6D's order, ids = its intensity):
 *   State (:2352-2358), fp64 from the store's float pose, rad2deg = 180.0 / M_PI (:197): yaw_k = (double)yaw * rad2deg in DEGREES and
 * t_k = (double)(x, y, z) are the 4 unknowns of position k; pitch_k, roll_k (likewise) are constants (the yaw block has size 1, :2361).
 *   Odometry edge (:2367-2373), one per position i >= 1, from i - 1: m = q_from^-1 (t_i - t_from) with q_from of the reference's chain (as
 * rgc_kf_assemble uses it), rel_yaw = yaw_i - yaw_from NOT normalised, pitch_from, roll_from -- built from the store's poses themselves.
 *   Loop edge (:2376-2392) from key_loop to key_curr: m = t_loop_curr, rel_yaw = yaw_loop_curr_deg (R2ypr(q_loop_curr).x), pitch / roll those
 * of keyPose6DLoop as recorded at detection.  A loop is USED when both its ids are selected and key_curr is not at position 0 (the `continue`
 * at :2364 precedes :2376); every other loop is ignored and counted.  "Both ids are selected" REPLACES the reference's membership test in
 * correctedKeyPose6DByLoop (:2338, 2386: the poses of the previous optimisation, which this library does not keep).  Unlike the reference's
 * loopInfoContainer (a map keyed by key_curr) several loops may end at one keyframe; at most RGC_PGO_MAX_LOOPS used loops (the reference
 * holds 100, :2110-2113).
 *   Residual of an edge i -> j (src/lidarFactor.hpp:557-595), NULL loss, cost = 1/2 sum |r|^2:  r[0..2] = R(yaw_i, pitch, roll)^T (t_j - t_i) - m
 * with YawPitchRollToRotationMatrix (:517-533, degrees in), r[3] = NormalizeAngle(yaw_j - yaw_i - rel_yaw) (:490-499: one wrap at +-180,
 * derivative 1).  Jacobians analytic: d r[0..2] / d yaw_i = (pi / 180) (dR/dyaw)^T (t_j - t_i), d r[3] / d yaw_i = -1, d r[0..2] / d t_i = -R^T,
 * d r[3] / d yaw_j = +1, d r[0..2] / d t_j = R^T.
 *   Gauge (:2325-2344, 2404-2414): the keyframe with the smallest key_loop id among the used loops is constant, all four parameters.  With no
 * used loop nothing is optimised and no pose changes (RGC_PGO_NO_LOOP; :2308, 2415-2419).
 *   Solve (:2423-2427): Ceres' trust-region LM as rgc_mapreg_optimize restates it, in dimension 4 (N - 1): damping clamp(diag H, 1e-6, 1e32) /
 * radius, a step is accepted above rho = 1e-3, the same radius update and the same four stops (gradient 1e-10, function 1e-6, parameter 1e-8
 * over the free parameters, radius 1e-32); a damped system that is not positive definite counts as a rejected step.  Plus is
 * NormalizeAngle(yaw + delta) on the yaw (:501-515), additive on t.  Ceres' Jacobi scaling is not restated (as in rgc_mapreg_optimize: parity
 * unpinned).  Every iteration linearises and solves the sparse system on the device, directly (nested dissection of the chain), in
 * fp64 with every sum in a fixed order: results are bit-identical from run to run.  The LM decisions are taken on the host.
 *   Write-back (:2450-2462): x, y, z = (float)t, yaw = (float)(yaw_deg * deg2rad); pitch and roll stay as stored, bit for bit.  The
 * reference's "loop pose changed by > 0.01" bail-out (:2441-2447) guards a Ceres defect; the constant node cannot move here, it is not reproduced.
 *   State machine: like the other rgc_kf_* calls these touch the store's poses and buffers of their own; with a solve in flight
 * (rgc_align_begin .. rgc_align_end) they RUN and the solve's result is what it would have been. */
enum { RGC_PGO_OPTIMIZED = 0, RGC_PGO_NO_LOOP = 1 };
enum { RGC_PGO_STOP_CAP = 0, RGC_PGO_STOP_GRADIENT = 1, RGC_PGO_STOP_FUNCTION = 2, RGC_PGO_STOP_PARAMETER = 3, RGC_PGO_STOP_RADIUS = 4 };
#define RGC_PGO_MAX_LOOPS 128
typedef struct rgc_pgo_loop {
  int key_curr, key_loop;          /* loopInfo::key_curr, key_loop (:2101-2102) */
  double t_loop_curr[3];           /* loopInfo::t_loop_curr (:2105) */
  double yaw_loop_curr_deg;        /* Utility::R2ypr(q_loop_curr.toRotationMatrix()).x() (:2389-2390) */
  double pitch_loop_deg, roll_loop_deg; /* keyPose6DLoop.pitch / roll * rad2deg (:2391) */
} rgc_pgo_loop;
typedef struct rgc_pgo_params {
  int max_iterations;              /* options.max_num_iterations (10, :2425) */
  double initial_radius;           /* ceres::Solver::Options::initial_trust_region_radius (1e4) */
} rgc_pgo_params;
typedef struct rgc_pgo_report {
  int status;                      /* RGC_PGO_OPTIMIZED | RGC_PGO_NO_LOOP */
  int n_nodes, n_odom, n_loops_used, n_loops_ignored;
  int fixed_id;                    /* oldestLoopKey (:2322-2344), -1 under RGC_PGO_NO_LOOP */
  int iterations, successful;      /* LM iterations run, accepted steps */
  int stop;                        /* RGC_PGO_STOP_* */
  unsigned accepted_mask;          /* bit k: the step of iteration k was accepted */
  double initial_cost, final_cost; /* 1/2 sum |r|^2 before / after */
} rgc_pgo_report;
RGC_API void rgc_default_pgo_params(rgc_pgo_params* p);
/* host only: the edge a loop-closure ICP gives (:2086-2107).  T_loop_correct = T_w_loop^-1 * T_drift * T_w_latest in fp32 with
 * pclPointToAffine3f (:2614-2617: pcl::getTransformation) of the two key poses and T_drift = rgc_icp_align's final_T (row-major 4x4);
 * t_loop_curr = its translation, yaw_loop_curr_deg = R2ypr of its linear part (widened to fp64), pitch / roll = the loop pose's * rad2deg.
 * (T_w_loop^-1 is formed as [R^T | -R^T t]; the reference's Eigen general inverse and its rotation() differ from that by fp32 rounding.) */
RGC_API int rgc_pgo_make_loop(const rgc_kf_pose* latest_pose, const rgc_kf_pose* loop_pose, const float T_drift[16], int key_curr, int key_loop,
                              rgc_pgo_loop* out);
/* reads the poses of ids[0 .. n_ids) from the keyframe store and optimises them.  params: NULL = defaults.  out_poses (nullable): the n_ids
 * corrected poses (the stored ones under RGC_PGO_NO_LOOP).  apply != 0 and RGC_PGO_OPTIMIZED: they are written back as rgc_kf_set_poses does,
 * all or nothing, the revision bumped once.  RGC_ERR_INVALID, nothing changed: an unknown or repeated id, n_ids < 1, a loop from a keyframe to
 * itself, more than RGC_PGO_MAX_LOOPS used loops, non-finite loop data, max_iterations outside 0..32 (accepted_mask has one bit per iteration: its
 * 32 bits are the only reason for that limit), a radius that is not positive. */
RGC_API int rgc_pgo_optimize(rgc_ctx* ctx, const int* ids, int n_ids, const rgc_pgo_loop* loops, int n_loops, const rgc_pgo_params* params,
                             int apply, rgc_kf_pose* out_poses, rgc_pgo_report* report);
/* what one LM iteration of rgc_pgo_optimize sees, read out (the counterpart of rgc_mapreg_linearize); every output is nullable.  The same
 * selection and loops; x_eval (nullable: the store's state): 4 n_ids doubles {yaw_deg, t} per position -- the edges are always built from the
 * store's poses.  Edges: the n_ids - 1 odometry edges first, then the used loops in the order given; edge_ij 2 ints (positions i, j),
 * edge_meas 6 doubles {m[3], rel_yaw, pitch, roll}, residuals 4 doubles per edge.  g: 4 n_ids (the constant node's rows zero).  H as 4x4
 * row-major blocks: H_diag n_ids of them, H_chain n_ids - 1 (block k: rows of position k, columns of k + 1, the odometry edge's term),
 * H_loop one per used loop (rows of key_loop's position, columns of key_curr's; that loop's term alone, also where two loops join the same
 * pair or the pair are neighbours -- the solve adds them onto the chain's block).  d (4 n_ids): the LM step of the system damped at radius,
 * written when radius > 0 and a loop is used.  report: status, counts and fixed_id; initial_cost = final_cost = the cost.  A damped system that is not
 * positive definite (a numerical condition, reported with the argument errors' code) is RGC_ERR_INVALID; on any error no output is written. */
RGC_API int rgc_pgo_linearize(rgc_ctx* ctx, const int* ids, int n_ids, const rgc_pgo_loop* loops, int n_loops, const double* x_eval, double radius,
                              int* edge_ij, double* edge_meas, double* residuals, double* g, double* cost, double* H_diag, double* H_chain,
                              double* H_loop, double* d, rgc_pgo_report* report);

/* ---- NDT registration (P2D / D2D) on a Gaussian voxel map: fast_gicp::NDTCuda (include/fast_gicp/ndt/ndt_cuda.hpp:27-60,
 * include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:10-90, src/fast_gicp/cuda/ndt_cuda.cu:13-177, src/fast_gicp/cuda/ndt_compute_derivatives.cu:33-231), the one
 * registration of the vendored tree whose only body is CUDA ----
 * A block of its own on the context, beside the VGICP clouds, the local map and the keyframe store: the rgc_ndt_* calls touch the NDT clouds,
 * their voxel maps and scratch of their own -- never a cloud or a solve of the registration above.  With a solve in flight (rgc_align_begin ..
 * rgc_align_end) every one of them RUNS and the solve's result is what it would have been.  The LM and convergence settings are the
 * context's rgc_params: max_iterations, lm_max_iterations, rotation_eps, translation_eps, lm_init_lambda_factor, max_cells.
 *   Voxel map (src/fast_gicp/cuda/gaussian_voxelmap.cu:122-148,178-198,209-231), resolution res: voxel of a point = floor(x / res - 0.5) per axis
 * (include/fast_gicp/cuda/vector3_hash.cuh:35-37, the VGICP map's coordinate); per voxel n, mean = sum p / n, cov = (sum p p^T - mean (sum p)^T) / n,
 * then MIN_EIG (src/fast_gicp/cuda/covariance_regularization.cu:83-100; src/fast_gicp/cuda/ndt_cuda.cu:128,139): every eigenvalue raised to at
 * least 1e-3.  Input points fp32, everything after them fp64; every per-voxel sum in ascending point index, every reduction in a fixed order:
 * results are bit-identical from run to run and between host- and device-pointer inputs.  Both maps are built lazily by the first call that
 * needs them (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:76-79), the source's only in D2D; RGC_ERR_NONFINITE / RGC_ERR_GRID_TOO_LARGE for a
 * cloud are therefore returned by that call.
 *   Terms (src/fast_gicp/cuda/find_voxel_correspondences.cu:55-60,92-110; src/fast_gicp/cuda/ndt_compute_derivatives.cu:50-91,120-163): for every
 * source element a -- a source point in P2D, the mean of a voxel of the source's own map in D2D -- and EVERY offset o of the neighbour
 * method, the voxel at coord(T a) + o if it exists and holds more than 6 points: e = mean_B - (R a + t); M = cov_B^-1 (P2D) or
 * (cov_B + R_lin cov_A R_lin^T)^-1 (D2D, R_lin the rotation of the last rgc_ndt_linearize); w = res^2 / (res^2 + |e|^2); cost += w e^T M e,
 * J = [skew(R a + t), -I], H += w J^T M J, b += w J^T M e.  RGC_NDT_DIRECT_RADIUS (src/fast_gicp/cuda/ndt_cuda.cu:70-84): all integer offsets
 * of [-ceil(r), ceil(r)]^3 with |o| <= r + 1e-3, in nested i, j, k order; at most RGC_NDT_MAX_OFFSETS of them (r < 4.9).
 *   Frozen terms: rgc_ndt_compute_error re-uses the (element, voxel) list and R_lin of the last rgc_ndt_linearize; the weights follow the pose
 * it is given (src/fast_gicp/cuda/ndt_cuda.cu:162-177).  A new neighbour method or radius between the two calls leaves the frozen list in force
 * (as rgc_set_params does for the VGICP list); a new resolution or distance mode, and setting, clearing or swapping a cloud, drop it
 * (rgc_ndt_compute_error: RGC_ERR_INVALID until the next rgc_ndt_linearize). */
enum { RGC_NDT_P2D = 0, RGC_NDT_D2D = 1 };                                           /* fast_gicp::NDTDistanceMode, include/fast_gicp/ndt/ndt_settings.hpp:6 */
enum { RGC_NDT_DIRECT27 = 0, RGC_NDT_DIRECT7 = 1, RGC_NDT_DIRECT1 = 2, RGC_NDT_DIRECT_RADIUS = 3 };  /* fast_gicp::NeighborSearchMethod, include/fast_gicp/gicp/gicp_settings.hpp:8 */
#define RGC_NDT_MAX_OFFSETS 512
typedef struct rgc_ndt_params {
  double resolution;       /* setResolution (1.0)            src/fast_gicp/cuda/ndt_cuda.cu:15,31-33 */
  int    distance_mode;    /* setDistanceMode (RGC_NDT_D2D)  src/fast_gicp/cuda/ndt_cuda.cu:21,27-29 */
  int    neighbor_method;  /* setNeighborSearchMethod (RGC_NDT_DIRECT7) src/fast_gicp/cuda/ndt_cuda.cu:22,35-88 */
  double neighbor_radius;  /* ... its radius, read under RGC_NDT_DIRECT_RADIUS only (0.0) */
} rgc_ndt_params;
RGC_API void rgc_default_ndt_params(rgc_ndt_params* p);
RGC_API int rgc_ndt_set_params(rgc_ctx* ctx, const rgc_ndt_params* params);
RGC_API int rgc_ndt_get_params(const rgc_ctx* ctx, rgc_ndt_params* params);
/* setInputTarget / setInputSource (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:50-73; src/fast_gicp/cuda/ndt_cuda.cu:95-113): x, y, z first, stride in
 * bytes, like rgc_set_target*.  The cloud is copied: a host cloud is on the device when the call returns, a device cloud is read in stream
 * order on rgc_stream(ctx) (what rgc_kf_assemble(..., on_device = 1) wrote is consumed where it lies).  1 <= n <= 2^27. */
RGC_API int rgc_ndt_set_target(rgc_ctx* ctx, const float* xyz, int n, int stride_bytes);
RGC_API int rgc_ndt_set_source(rgc_ctx* ctx, const float* xyz, int n, int stride_bytes);
RGC_API int rgc_ndt_set_target_device(rgc_ctx* ctx, const float* d_xyz, int n, int stride_bytes);
RGC_API int rgc_ndt_set_source_device(rgc_ctx* ctx, const float* d_xyz, int n, int stride_bytes);
/* clearSource / clearTarget / swapSourceAndTarget (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:34-48; src/fast_gicp/cuda/ndt_cuda.cu:90-93: the clouds
 * and their voxel maps change roles) */
RGC_API int rgc_ndt_clear_source(rgc_ctx* ctx);
RGC_API int rgc_ndt_clear_target(rgc_ctx* ctx);
RGC_API int rgc_ndt_swap_source_and_target(rgc_ctx* ctx);
/* linearize / compute_error (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:81-90): T row-major 4x4; H, b as rgc_linearize (both or neither) */
RGC_API int rgc_ndt_linearize(rgc_ctx* ctx, const double T[16], double H[36], double b[6], double* cost);
RGC_API int rgc_ndt_compute_error(rgc_ctx* ctx, const double T[16], double* cost);
RGC_API int rgc_ndt_num_correspondences(rgc_ctx* ctx, int* n_terms);   /* terms of the last rgc_ndt_linearize */
/* computeTransformation (include/fast_gicp/ndt/impl/ndt_cuda_impl.hpp:75-79): LsqRegistration's driver as rgc_align runs it (lsq_registration_impl.hpp:53-79,
 * LM step :125-172), outputs as rgc_align's.  Any output pointer may be NULL. */
RGC_API int rgc_ndt_align(rgc_ctx* ctx, const float guess[16], float final_T[16], double final_H[36], int* iterations, int* converged, int* lm_failed);
/* voxel map read-out, which = 0 target, 1 source (built if need be, in either mode): up to cap voxels, unordered; coords 3*cap ints, n cap ints,
 * mean 3*cap doubles, cov9 9*cap doubles (after MIN_EIG); *count = total voxels.  rgc_ndt_get_raw_covariances: the covariances BEFORE MIN_EIG,
 * in the same voxel order. */
RGC_API int rgc_ndt_get_voxels(rgc_ctx* ctx, int which, int cap, int* coords, int* n, double* mean, double* cov9, int* count);
RGC_API int rgc_ndt_get_raw_covariances(rgc_ctx* ctx, int which, int cap, double* cov9, int* count);

/* ---- FastGICP: GICP on exact nearest-neighbour correspondences: fast_gicp::FastGICP (include/fast_gicp/gicp/fast_gicp.hpp:25-87,
 * include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:103-237), the registration FastVGICP derives from ----
 * On the context's OWN source and target (rgc_set_source* / rgc_set_target*, as FastVGICP inherits FastGICP's clouds) and their covariances as
 * they are: computed from the k nearest neighbours on either covariance route, or given by rgc_set_source_covariances / rgc_set_target_covariances.
 * No second copy of a cloud, no voxel look-up.  A lazy target is completed first; re-framed, borrowed (rgc_share_target) and map-bound targets
 * are used where they lie.  With a solve in flight (rgc_align_begin .. rgc_align_end) these calls are refused like the getters
 * (RGC_ERR_INVALID).  No source, no target, a NULL or non-finite pose: RGC_ERR_INVALID.  The LM and convergence settings are the context's rgc_params.
 *   For a pose T (row-major 4x4) and every source point p_i (include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:115-211):
 *   q = float(T) p_i in fp32, ((m0 x + m1 y) + m2 z) + m3, never contracted (:119,131); j = the target point with the smallest fp32
 * ((dx dx + dy dy) + dz dz), ties to the smaller index (:133); kept iff (double)key < d_max^2 (:136, strict).  For a kept pair, in fp64:
 * a = R p_i + t, e = b_j - a, M = (C_B[j] + R C_A[i] R^T)^-1 (the 3x3 block of :146-150), cost += e^T M e, J = [skew(a), -I],
 * H += J^T M J, b += J^T M e (:179-198).  Every reduction runs in a fixed order: results are bit-identical from run to run and between
 * host- and device-pointer inputs.  No kept pair: cost 0, H = 0, b = 0.
 *   Frozen cost: rgc_gicp_compute_error re-uses the pairs and the M of the last rgc_gicp_linearize at the pose it is given (:214-237).
 * Setting, clearing or swapping a cloud, setting covariances and a setting that prepares a cloud again drop them (RGC_ERR_INVALID until the
 * next rgc_gicp_linearize); a new maximum distance does not. */
RGC_API int rgc_gicp_set_max_correspondence_distance(rgc_ctx* ctx, double d_max);   /* setMaxCorrespondenceDistance; default FLT_MAX (:18): nothing rejected; >= 0 */
RGC_API int rgc_gicp_get_max_correspondence_distance(const rgc_ctx* ctx, double* d_max);
/* linearize / compute_error: H, b as rgc_linearize (both or neither) */
RGC_API int rgc_gicp_linearize(rgc_ctx* ctx, const double T[16], double H[36], double b[6], double* cost);
RGC_API int rgc_gicp_compute_error(rgc_ctx* ctx, const double T[16], double* cost);
RGC_API int rgc_gicp_num_correspondences(rgc_ctx* ctx, int* n_kept);               /* kept pairs of the last rgc_gicp_linearize */
/* the pairs of the last rgc_gicp_linearize in caller order, n_source entries each (either may be NULL): idx = the target point's index or -1
 * where rejected, sq_dist = the key even where rejected (:135) */
RGC_API int rgc_gicp_get_correspondences(rgc_ctx* ctx, int* idx, float* sq_dist);
/* computeTransformation (:103-112): LsqRegistration's driver as rgc_align's host route runs it (lsq_registration_impl.hpp:53-79, LM step :125-172),
 * outputs as rgc_align's.  Any output pointer may be NULL. */
RGC_API int rgc_gicp_align(rgc_ctx* ctx, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged,
                           int* lm_failed);

/* ---- FastGICPSingleThread: GICP with anchor-cached correspondences: fast_gicp::FastGICPSingleThread (include/fast_gicp/gicp/fast_gicp_st.hpp:20-65,
 * include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:19-125), the FastGICP that searches a point again only when it has to ----
 * On the context's OWN source and target and their covariances as they are, exactly as rgc_gicp_* (either covariance route, caller-set
 * covariances, lazy -- completed first --, re-framed, borrowed and map-bound targets); refused with a solve in flight; no source, no target, a
 * NULL or non-finite pose: RGC_ERR_INVALID.  d_max is FastGICP's own setting (rgc_gicp_set_max_correspondence_distance); the LM and convergence
 * settings are the context's rgc_params.  It is NOT FastGICP with a faster search: a point that is not searched again keeps its pair, its keys
 * and its Mahalanobis matrix from the pose it was last searched at, so the numbers differ from rgc_gicp_*'s.
 *   State per source point: corr, key1, key2 (fp32), the anchor (3 fp32), M (6 fp64).  For a pose T (row-major 4x4) and every source point p_i
 * (citations: fast_gicp_st_impl.hpp):
 *   q = float(T) p_i in fp32, ((m0 x + m1 y) + m2 z) + m3, never contracted (:44).  If the point has an anchor a_i (:46-54): d2 = (dx dx + dy dy)
 * + dz dz of q - a_i in fp32, d = (double)(float)sqrt((double)d2), max_first = (double)(float)sqrt((double)key1) + d, min_second =
 * (double)(float)sqrt((double)key2) - d; the point is SKIPPED iff max_first < min_second (:51, strict, fp64) and everything it has stays.
 * Otherwise it is SEARCHED (:56-75): key1 = the smallest fp32 key ((dx dx + dy dy) + dz dz) over the target and j its point, ties to the smaller
 * index, exactly as rgc_gicp_*; key2 = the second smallest key of the multiset (== key1 where the nearest is tied or duplicated; +INF when the
 * target has one point -- the reference reads a stale value there); corr = j iff (double)key1 < d_max^2 (:58, strict) else -1; the anchor
 * becomes q (:61); for a kept pair M = (C_B[j] + R C_A[i] R^T)^-1 at THIS pose (:67-75).  Then FastGICP's term for every pair with corr >= 0
 * under the stored M (:80-120).  As in the reference a skipped point keeps its pair (or its -1) after it crosses d_max.  Every reduction runs in
 * a fixed order: results are bit-identical from run to run and between host- and device-pointer inputs.
 *   Frozen cost: rgc_gicpst_compute_error is the cost of the state as it is at the pose it is given (:122-125).
 *   The state (anchors included) drops on rgc_gicpst_reset, at the start of rgc_gicpst_align (:19-22) and wherever FastGICP's frozen list drops;
 * the next linearisation then searches every point, and until then the read-outs and rgc_gicpst_compute_error are RGC_ERR_INVALID.  A new
 * d_max does not drop it.  Deviations from the reference: DESIGN.md section 6. */
RGC_API int rgc_gicpst_reset(rgc_ctx* ctx);
/* H, b as rgc_gicp_linearize (both or neither); cost nullable */
RGC_API int rgc_gicpst_linearize(rgc_ctx* ctx, const double T[16], double H[36], double b[6], double* cost);
RGC_API int rgc_gicpst_compute_error(rgc_ctx* ctx, const double T[16], double* cost);
RGC_API int rgc_gicpst_num_correspondences(rgc_ctx* ctx, int* n_kept);             /* pairs with corr >= 0 after the last rgc_gicpst_linearize */
RGC_API int rgc_gicpst_num_searched(rgc_ctx* ctx, int* n_searched);                /* points the last rgc_gicpst_linearize searched */
/* the state after the last rgc_gicpst_linearize in caller order, n_source entries each (any may be NULL): idx = the target point's index or -1,
 * sq_dist / second_sq_dist = key1 / key2 at the point's anchor, searched = 1 where the last linearisation searched the point, else 0 */
RGC_API int rgc_gicpst_get_correspondences(rgc_ctx* ctx, int* idx, float* sq_dist, float* second_sq_dist, int* searched);
/* outputs as rgc_gicp_align's (any may be NULL) */
RGC_API int rgc_gicpst_align(rgc_ctx* ctx, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged,
                             int* lm_failed);

/* ---- FastGICPMultiPoints: GICP on radius-merged target distributions: fast_gicp::FastGICPMultiPoints
 * (include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp:40-53, include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:92-221) ----
 * The one registration of the family whose correspondence is a RADIUS SEARCH: every source point is matched against the distance-weighted merge of
 * every target Gaussian within neighbor_search_radius of it.  On the context's OWN source and target and their covariances as they are, exactly as
 * rgc_gicp_* (either covariance route, caller-set covariances, lazy -- completed first --, re-framed, borrowed and map-bound targets); refused with a
 * solve in flight; no source, no target, a NULL or non-finite pose: RGC_ERR_INVALID.  (The entry points are rgc_gicpmp_*: the prefix rgc_gicp_ is
 * FastGICP's own set.)
 *   For a pose T (row-major 4x4) and every source point p_i (citations: fast_gicp_mp_impl.hpp):
 *   q = float(T) p_i in fp32, ((m0 x + m1 y) + m2 z) + m3, never contracted (:141).  N_i = every target point j whose fp32 key
 * ((dx dx + dy dy) + dz dz) < r2, strict, r2 = (float)((double)r * (double)r) -- pcl::KdTreeFLANN::radiusSearch's rule (:145); nothing capped,
 * nothing approximated.  w_j = max(1e-3, min(1, 1 - (double)(float)sqrt((double)key_j) / r)) (:184-185).  In fp64: sw = sum w_j, mean_B =
 * sum w_j b_j / sw, cov_B = sum w_j C_B[j] / sw (:180-195; the reference's casts of the two to fp32 are not made).  A point with an empty N_i is
 * skipped (:176).  For the others a = R p_i + t, d = mean_B - a, M = (cov_B + R C_A[i] R^T)^-1 (the 3x3 block of :199-202), loss l = M d, J =
 * M [skew(a) | -I] (:203-213); the system is plain Gauss-Newton over those rows: with D = [skew(a) | -I] and W = M M, cost = sum d^T W d, H = sum
 * D^T W D, b = sum D^T W d -- M SQUARED, the reference's definition.  Every sum runs in a fixed order: results are bit-identical from run to run
 * and between host- and device-pointer inputs.
 *   rgc_gicpmp_align (:92-108): up to max_iterations times linearise at T, solve H delta = -b (undamped, the host LM driver's 6x6 factorisation),
 * T <- [so3_exp(delta_r) | delta_t] T; converged (:118-127) when max(|so3_exp(delta_r) - I|_max / rotation_epsilon, |delta_t|_max /
 * transformation_epsilon) < 1, tested after the update.  iterations = linearisations made.  A refused or non-finite solve, or no source point with
 * a neighbour: the solve stops at the last good pose with failed = 1 (the status is RGC_OK, as rgc_gicp_align reports lm_failed).  Deviations from
 * the reference (its update of the pose, its missing solver, its un-normalised covariances, neighbour order, fp64): DESIGN.md section 6.
 *   The kept results (rgc_gicpmp_num_correspondences, _get_merged, _get_neighbors) are those of the last linearisation; they drop wherever
 * FastGICP's frozen list drops, and on rgc_gicpmp_set_params (RGC_ERR_INVALID until the next linearisation). */
typedef struct rgc_gicp_mp_params {
  double neighbor_search_radius;   /* neighbor_search_radius_ (0.5)  fast_gicp_mp_impl.hpp:35; finite, > 0, float(r r) finite */
  int    max_iterations;           /* max_iterations_ (64)           fast_gicp_mp_impl.hpp:29; >= 1 */
  double rotation_epsilon;         /* rotation_epsilon_ (1e-5)       fast_gicp_mp_impl.hpp:30; > 0 */
  double transformation_epsilon;   /* transformation_epsilon_ (1e-5) fast_gicp_mp_impl.hpp:31; > 0 */
} rgc_gicp_mp_params;
RGC_API void rgc_default_gicp_mp_params(rgc_gicp_mp_params* p);
RGC_API int rgc_gicpmp_set_params(rgc_ctx* ctx, const rgc_gicp_mp_params* p);
RGC_API int rgc_gicpmp_get_params(const rgc_ctx* ctx, rgc_gicp_mp_params* p);
/* H, b as rgc_gicp_linearize (both or neither); cost nullable */
RGC_API int rgc_gicpmp_linearize(rgc_ctx* ctx, const double T[16], double H[36], double b[6], double* cost);
/* of the last linearisation: the source points with at least one neighbour, and the total of |N_i| (either may be NULL) */
RGC_API int rgc_gicpmp_num_correspondences(rgc_ctx* ctx, int* n_points, long long* n_pairs);
/* of the last linearisation: the target points the gather looked at over all source points (the members of every grid row range a ball reaches):
 * what the pairs cost to find */
RGC_API int rgc_gicpmp_num_candidates(rgc_ctx* ctx, long long* n_candidates);
/* per source point in caller order, n_source entries each (any may be NULL): |N_i|, sw, mean_B (3), cov_B (6: xx xy xz yy yz zz); where count is 0
 * the other three are zeros */
RGC_API int rgc_gicpmp_get_merged(rgc_ctx* ctx, int* count, double* sum_w, double* mean3, double* cov6);
/* the rows N_i in CSR form, caller order: offsets (n_source + 1 entries), idx (original target indices) and sq_dist (the fp32 keys), cap entries
 * each.  The order inside a row is unspecified but the same from run to run.  *n_total = the total whatever cap is; cap < *n_total:
 * RGC_ERR_INVALID and no row is written. */
RGC_API int rgc_gicpmp_get_neighbors(rgc_ctx* ctx, int* offsets, int* idx, float* sq_dist, int cap, long long* n_total);
/* outputs as rgc_gicp_align's (any may be NULL); final_H = the H of the last step taken (identity if none) */
RGC_API int rgc_gicpmp_align(rgc_ctx* ctx, const float guess[16], float final_T[16], double final_H[36], double* fitness, int* iterations, int* converged,
                             int* failed);

/* ---- the search index: exact k nearest neighbours and radius search of arbitrary queries: pcl::KdTreeFLANN::nearestKSearch / radiusSearch as the
 * reference calls them (src/RGC_mapping.cpp:1097,1147,1196,1243: 5-NN in the corner and surf maps; src/RGC_mapping.cpp:1537,2157: radius search over
 * the key poses; include/fast_gicp/gicp/impl/fast_gicp_impl.hpp:133,254; include/fast_gicp/gicp/impl/fast_gicp_st_impl.hpp:56;
 * include/fast_gicp/gicp/impl/fast_vgicp_cuda_impl.hpp:161; include/fast_gicp/gicp/experimental/fast_gicp_mp_impl.hpp:145,148,233) ----
 * The index is a cloud of the context's OWN: rgc_search_set_cloud copies a host cloud, or counting-sorts a device cloud into the library's buffer (the
 * input need not stay alive after the call returns), and builds a grid over its measured box.  It is independent of the context's source and target
 * and of every other subsystem; a solve in flight refuses its calls (RGC_ERR_INVALID).  n <= 2^27 points.
 *   Key: the fp32 ((dx dx + dy dy) + dz dz), never FMA-contracted -- flann::L2_Simple<float>, the key of every other search of this library; sq_dist
 * returns it.  Order: ascending (key, original index), a total order: a row is unique whatever the grid, the cell size or the launch shape, and results
 * are bit-identical from run to run and between host and device pointers.
 *   rgc_search_knn: k in 1..RGC_SEARCH_MAX_K.  Row i (k entries) holds the min(k, n) smallest of query i under that order; entries behind min(k, n)
 * are idx = -1, sq_dist = +inf (PCL shrinks k to n; a fixed row width with a sentinel is this library's form of that).
 *   rgc_search_radius: a point is a member iff key < r2, strict, r2 = (float)((double)radius * (double)radius) -- the rule rgc_gicpmp_* documents for
 * pcl::KdTreeFLANN::radiusSearch; radius finite and > 0, r2 finite.  max_nn = 0: every member, nothing capped.  max_nn in 1..RGC_SEARCH_MAX_K: the
 * max_nn smallest members under the order (FLANN's bounded result set under an exact search); a larger max_nn is RGC_ERR_INVALID.  Rows are CSR:
 * offsets (nq + 1 entries), idx and sq_dist (cap entries each; sq_dist nullable).  sorted != 0: rows ascending under the order (PCL's default,
 * sorted_results_ = true); sorted = 0: the order inside a row is unspecified (the grid's: it moves with the cell size) but the same from run to run.  *n_total is always the total;
 * cap < *n_total: RGC_ERR_INVALID, no row and no offset written, *n_total still set (rgc_gicpmp_get_neighbors' protocol: size the second call with
 * it).  A total beyond 2^31 - 1 is RGC_ERR_INVALID too (the offsets are 32-bit).
 *   on_device covers the queries AND the outputs, as in rgc_kf_assemble: all host memory or all device memory of the context's GPU.
 *   Refusals: no index: RGC_ERR_NO_INPUT; nq = 0: RGC_OK (offsets[0] = 0); nq < 0, k or max_nn out of range, a bad stride, a NULL it needs:
 * RGC_ERR_INVALID; a non-finite coordinate in the indexed cloud or in a query: RGC_ERR_NONFINITE, detected on the device (the grid build's flag
 * word; a query kernel searches nothing for such a query and raises a flag) -- no output is written, and for the cloud the context holds no index.
 *   cell: > 0 is the grid's cell size as given (RGC_ERR_GRID_TOO_LARGE as elsewhere, rgc_params::max_cells); 0 selects it: the box's extent is
 * measured in cells of 1 m (of 1/16 m when no axis spans more than 8 of those), cell = the power of two nearest cbrt(4 V / n) with V the product of
 * the three extents (about four points per cell of a filled box), within [2^-8, 2^16] m, doubled while the grid would hold more than
 * max(4 n, 4096) cells.  Results never depend on it.
 *   rgc_search_get_info: the index, and what the LAST query call cost: the indexed points it looked at, the queries whose cube of cells grew beyond
 * its first size (the 3 x 3 x 3 block about the query's cell; rgc_search_knn and a bounded radius search), the rows that took the sort's long route
 * (an uncapped sorted radius search; rows up to rgc_search_sort_window() members are sorted in one pass). */
#define RGC_SEARCH_MAX_K 32
typedef struct rgc_search_info {
  int n;                       /* points indexed (0: no index)                                    */
  double cell;                 /* the grid's cell size in use                                     */
  long long cells;             /* cells of the grid                                               */
  long long candidates;        /* last query call: indexed points looked at over all queries      */
  int grown;                   /* last query call: queries whose cube of cells had to grow        */
  int rows_sorted_long;        /* last query call: radius rows longer than the sort window        */
} rgc_search_info;
RGC_API int rgc_search_set_cloud(rgc_ctx* ctx, const float* xyz, int n, int stride_bytes, int on_device, double cell);
RGC_API int rgc_search_clear(rgc_ctx* ctx);
RGC_API int rgc_search_get_info(rgc_ctx* ctx, rgc_search_info* info);
/* host code, no context */
RGC_API int rgc_search_sort_window(void);
RGC_API int rgc_search_knn(rgc_ctx* ctx, const float* queries, int nq, int stride_bytes, int on_device, int k, int* idx, float* sq_dist);
RGC_API int rgc_search_radius(rgc_ctx* ctx, const float* queries, int nq, int stride_bytes, int on_device, double radius, int max_nn, int sorted,
                              int* offsets, int* idx, float* sq_dist, long long cap, long long* n_total);

/* ---- the outlier filters: pcl::StatisticalOutlierRemoval (SOR) and pcl::RadiusOutlierRemoval (ROR) of a cloud against itself, the two filters a
 * PCL-based LiDAR pipeline runs before a cloud goes into a map.  (The reference's three nodes do not call them; they complete the PCL filter family
 * beside rgc_voxelgrid and rgc_uniform_sampling.) ----
 *   Argument rules, on_device and the record format are rgc_uniform_sampling's: x, y, z as floats at the head of each record of stride_bytes; on_device
 * covers the cloud AND every output (all host memory or all device memory of the context's GPU); out_xyzc receives 16-byte records x, y, z, c that go
 * out unchanged (c = the float behind z, 0 for a 12-byte stride); out_index the kept points' input indices; both need room for n entries and either
 * may be NULL.  The output is in ASCENDING INPUT INDEX: PCL keeps the input's order.  *n_out = points kept.
 *   The filters build a grid of their own over the cloud (the search index's machinery and its automatic cell rule): a caller's search index, source
 * and target are untouched.  A solve in flight refuses the calls (RGC_ERR_INVALID), as it refuses the search index.  rgc_outlier_set_cell fixes the
 * grid's cell size for tests and tuning (0 = automatic; finite and >= 0); NO OUTPUT BIT DEPENDS ON IT, mean / stddev / threshold included.
 *   Key: the fp32 ((dx dx + dy dy) + dz dz), never FMA-contracted, as everywhere in this library.
 *   rgc_outlier_statistical -- restated from PCL's filters/impl/statistical_outlier_removal.hpp FROM MEMORY [3P-memory] (PCL is not available to this
 * project):
 *   Row: for point i the mean_k + 1 smallest keys over the whole cloud, the point itself included.  Entry 0 is dropped: it is the point itself or a
 * duplicate of it, either way the key 0 PCL drops as "k = 0 is the query point".
 *   Mean distance: d_i = (float)(sum over r = 1 .. mean_k of (double)sqrtf(key_r) / mean_k), the sum in fp64 in ascending rank (tied keys have equal
 * roots: the sum is unique), sqrtf the correctly rounded fp32 root.  out_mean_dist (nullable, n floats) receives d.
 *   Statistics: sum = sum of d_i, sq_sum = sum of (double)d_i (double)d_i (exact in fp64), both summed IN INPUT-INDEX ORDER in a fixed order: bit-identical
 * from run to run and independent of the grid.  mean = sum / n, variance = (sq_sum - sum sum / n) / (n - 1) clamped at 0, stddev = sqrt(variance),
 * threshold = mean + std_mul stddev, computed on the device.
 *   Decision: point i is kept iff (double)d_i <= threshold; with negative != 0 iff (double)d_i > threshold.
 *   Deviations from PCL: PCL sums sequentially and squares in fp32 before widening -- here fp64 after the key, as everywhere in this library; PCL takes
 * the root of a negative rounding residue (NaN: every point removed) -- here the variance is clamped; PCL reads past the row when n <= mean_k -- here
 * that is refused.  A hazard PCL shares and this library does not fix: when every d_i is equal and n is no power of two, mean may round one ulp under
 * d, and every point then counts as an outlier.
 *   Refusals: mean_k outside 1..RGC_OUTLIER_MAX_MEAN_K, n < 0, 0 < n < 2, n <= mean_k, a non-finite std_mul, a bad stride, a NULL cloud or n_out:
 * RGC_ERR_INVALID; n = 0: RGC_OK with *n_out = 0; a non-finite coordinate: RGC_ERR_NONFINITE, detected on the device, nothing written;
 * RGC_ERR_GRID_TOO_LARGE as elsewhere.
 *   rgc_outlier_radius [3P-memory: filters/impl/radius_outlier_removal.hpp]:
 *   Count: count_i = the cloud's points with key < r2, strict, r2 = (float)((double)radius * (double)radius) -- rgc_search_radius' membership rule; the
 * point itself is a member.  Point i is kept iff count_i - 1 >= min_neighbors; negative inverts this.  out_count (nullable, n ints) requested: the exact
 * count_i of every point; not requested: a point's walk may stop once its count exceeds min_neighbors (the same set is kept).
 *   Ranges: radius finite and > 0, r2 finite, min_neighbors >= 0 (RGC_ERR_INVALID); the other refusals as above, and n >= 1 suffices.
 *   Deviation from PCL: its dense-cloud shortcut (nearestKSearch(min_pts + 1) and <= against r^2) counts a neighbour exactly on the radius as inside,
 * its radiusSearch route does not; this library uses the strict rule on every route.
 *   rgc_outlier_get_info: the LAST filter call. */
#define RGC_OUTLIER_MAX_MEAN_K 63
typedef struct rgc_outlier_info {
  int n, n_out;                   /* points in, points kept                                       */
  double mean, stddev, threshold; /* SOR only (0 for ROR): of the mean distances, as the device computed them */
  double cell;                    /* the grid the call used: its cell size                        */
  long long cells;                /* ... and its cells                                            */
  long long candidates;           /* indexed points looked at over all points                     */
  int grown;                      /* SOR: points whose cube of cells had to grow                  */
} rgc_outlier_info;
RGC_API int rgc_outlier_statistical(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, int on_device, int mean_k, double std_mul, int negative,
                                    float* out_xyzc /* nullable */, int* out_index /* nullable */, float* out_mean_dist /* nullable, n */, int* n_out);
RGC_API int rgc_outlier_radius(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, int on_device, double radius, int min_neighbors, int negative,
                               float* out_xyzc /* nullable */, int* out_index /* nullable */, int* out_count /* nullable, n */, int* n_out);
RGC_API int rgc_outlier_get_info(rgc_ctx* ctx, rgc_outlier_info* info);
RGC_API int rgc_outlier_set_cell(rgc_ctx* ctx, double cell);

/* ---- Euclidean cluster extraction: pcl::EuclideanClusterExtraction of a cloud, the first structural operation a LiDAR pipeline runs on one (small
 * clusters dropped as noise before a scan goes into a map, movable objects cut out of a keyframe, what is left after the ground is removed).  (The
 * reference's three nodes do not call the PCL class, as they do not call the outlier filters; it completes the per-point PCL toolbox beside
 * rgc_search_* and rgc_outlier_*.) ----
 *   rgc_cluster_extract -- restated from PCL's segmentation/impl/extract_clusters.hpp FROM MEMORY [3P-memory] (PCL is not available to this project):
 *   Graph: points i and j are joined iff key(i, j) < r2, strict, r2 = (float)((double)tolerance * (double)tolerance) -- rgc_search_radius' and
 * rgc_outlier_radius' membership rule.  Key: the fp32 ((dx dx + dy dy) + dz dz), never FMA-contracted, as everywhere in this library; it is exactly
 * symmetric in fp32, so the graph is undirected and its connected components are well defined.  Duplicates (key 0) are always joined.
 *   Clusters: PCL grows a cluster from the lowest unprocessed index by breadth-first radiusSearch, marks everything it reaches as processed whether or
 * not the cluster is then kept, sorts the cluster's indices and keeps it iff min_size <= size <= max_size, both inclusive.  Hence a cluster IS a
 * connected component; a component over max_size is dropped whole, and its points go to no other cluster.
 *   Order: clusters by size descending, then by smallest member index ascending (a total order); members inside a cluster in ascending input index.
 * No output bit depends on the grid, on its cell size, on the launch shape or on the run; host-pointer and device-pointer calls give identical bytes.
 *   Outputs (each nullable): labels[i], i < n = the rank of i's cluster in that order, or -1 when the point is in no kept cluster; offsets[0 ..
 * n_clusters] and indices[0 .. n_clustered) = the clusters in CSR form (cluster r is indices[offsets[r] .. offsets[r + 1])).  Entries behind those ranges
 * are left untouched.  labels and indices need room for n ints, offsets for n + 1: a cluster table is never longer, which spares the size-then-fill
 * protocol of rgc_search_radius.  *n_clusters = clusters kept.
 *   Argument rules, on_device and the record format are rgc_outlier_radius': x, y, z as floats at the head of each record of stride_bytes; on_device
 * covers the cloud AND every output; n <= 2^27.  The call builds a grid of its own over the cloud (the search index's machinery and automatic cell
 * rule): a caller's search index, source and target are untouched.  A solve in flight refuses the call (RGC_ERR_INVALID).  rgc_cluster_set_cell fixes
 * the grid's cell size for tests and tuning (0 = automatic; finite and >= 0); NO OUTPUT BIT DEPENDS ON IT.
 *   Refusals: tolerance not finite or <= 0, r2 not finite, min_size < 1, max_size < min_size, n < 0, a bad stride, a NULL cloud (n > 0), context or
 * n_clusters: RGC_ERR_INVALID; n = 0: RGC_OK with zero clusters and offsets[0] = 0 if offsets is given; a non-finite coordinate: RGC_ERR_NONFINITE,
 * detected on the device by the grid build, nothing written; RGC_ERR_GRID_TOO_LARGE as elsewhere; RGC_ERR_HIP with a message and nothing written
 * should a union-find loop of the linking kernels ever run past its iteration cap (a logic error surfaces as a code, not as a kernel that does not end).
 * PCL's defaults (min_size 1, max_size INT_MAX) are accepted.
 *   Deviations from PCL: the order among clusters of equal size -- PCL's final unstable std::sort by size leaves ties unspecified, here the smaller
 * smallest member index goes first; PCL's optional indices-subset input and ConditionalEuclideanClustering are not built.
 *   rgc_cluster_get_info: the LAST rgc_cluster_extract. */
typedef struct rgc_cluster_info {
  int n;                 /* points in                                                     */
  int n_components;      /* connected components before the size limits                   */
  int n_clusters;        /* components kept                                               */
  int n_clustered;       /* points in kept clusters                                       */
  int largest;           /* size of the largest component, kept or not                    */
  double cell;           /* the grid the call used: its cell size                         */
  long long cells;       /* ... and its cells                                             */
  long long candidates;  /* indexed points looked at over all points (as rgc_outlier_info) */
} rgc_cluster_info;
RGC_API int rgc_cluster_extract(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, int on_device, double tolerance, int min_size, int max_size,
                                int* labels /* nullable, n */, int* offsets /* nullable, n + 1 */, int* indices /* nullable, n */, int* n_clusters);
RGC_API int rgc_cluster_get_info(rgc_ctx* ctx, rgc_cluster_info* info);
RGC_API int rgc_cluster_set_cell(rgc_ctx* ctx, double cell);

/* ---- RANSAC plane segmentation: pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC, setOptimizeCoefficients, and the
 * pcl::ExtractIndices step behind it -- the ground removal between the outlier filters and rgc_cluster_extract ("what is left after the ground is
 * removed").  (The reference's three nodes do not call the PCL class; its only plane fit is the front-end's ring-tabulated ground stage.)  The result is a
 * pure function of the cloud, the parameters and the seed: no output bit depends on the launch shape, the batch size or the run. ----
 *   rgc_plane_segment -- PCL's part restated FROM MEMORY [3P-memory] (PCL is not available to this project).
 *   Record format and on_device are rgc_outlier_radius': x, y, z as floats at the head of each record of stride_bytes; on_device covers the cloud,
 * out_xyzc and out_index; coeff, n_out, out_counts, samples and the info are always host memory; n <= 2^27.  No grid is built.  A solve in flight
 * refuses the call (RGC_ERR_INVALID).
 *   Hypothesis stream: stream position t = 0, 1, 2, ... yields a triple (i0, i1, i2) of distinct point indices.  With samples != NULL (host, 3 *
 * n_samples ints) position t is samples[3t .. 3t + 2] and the stream ends at n_samples; an index outside [0, n) or two equal indices in a triple is
 * RGC_ERR_INVALID before anything runs.  Otherwise (n_samples is ignored) the triple is rgc_plane_sample(seed, t, n) and the stream ends at 10 *
 * max_iterations.  rgc_plane_sample is a counter-based generator, a pure host function (no context, no GPU: rgc_neighbor_offsets' precedent), in
 * unsigned 64-bit arithmetic (mod 2^64):
 *     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     r_j = mix(seed + (3 t + j + 1) * 0x9E3779B97F4A7C15), j = 0, 1, 2        (splitmix64 started at seed: its outputs 3t + 1 .. 3t + 3)
 *     i0 = r_0 % n;   i1 = (i0 + 1 + r_1 % (n - 1)) % n;   i2 = the (r_2 % (n - 2))-th index, counting from 0 ascending, not in {i0, i1}
 * -- distinct by construction, never a retry.  n < 3 or a NULL ijk: RGC_ERR_INVALID.
 *   Model of a triple, in fp64 from the fp32 points p0, p1, p2, in this operation order, never FMA-contracted:
 *     e1 = p1 - p0, e2 = p2 - p0;   c = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x);   u.v stands for (ux vx + uy vy) + uz vz
 *     n = c / sqrt(c.c) (three divisions);   d = -(n.p0);   the stored model is ((float)nx, (float)ny, (float)nz, (float)d).
 * A position is INVALID, and counts as skipped, iff !(c.c > 1e-12 * ((e1.e1) * (e2.e2))) (collinear or coincident), or n, d or a stored value is not
 * finite, or -- model_type = RGC_PLANE_PERPENDICULAR [3P-memory: SampleConsensusModelPerpendicularPlane, the normal within eps_angle of the axis] --
 * fabs(n.a) < cos(eps_angle) in fp64, a = axis / sqrt(axis.axis).
 *   Score: point p is an inlier of a model (a, b, c, d) iff fabsf(((a x + b y) + c z) + d) < thr, STRICT, in fp32, never FMA-contracted, thr =
 * (float)distance_threshold -- the library's strict rule.  The score of a position is its inlier count over the whole cloud.
 *   Decision: the sequential loop over the stream [3P-memory: sample_consensus/impl/ransac.hpp].  best = -1, k = 1, iterations = 0, skipped = 0.  At each
 * position: an invalid one adds to skipped only.  A valid one with count > best (strict: the earlier position wins a tie) becomes the best; then w =
 * (double)best / n, q = min(max(1 - (w w) w, DBL_EPSILON), 1 - DBL_EPSILON), k = log(1 - probability) / log(q) in fp64 on the host; then ++iterations,
 * and the loop stops if iterations >= k or iterations == max_iterations.  The loop also stops behind the stream's last position.  The positions are
 * scored in batches and the loop is replayed over their counts: positions evaluated past the stop are ignored, so the result is the same for every
 * batch size.  Deviations from PCL: PCL allows max_iterations + 1 iterations; PCL draws its samples with rand() (and redraws, up to a cap, a sample
 * its isSampleGood rejects, which tests coordinate RATIOS where this tests the cross product); PCL's skipped-count limit is this stream end.
 *   Inliers and refinement: the inliers are the points within the rule of the best model, in ascending input index.  optimize != 0 and at least 3
 * inliers [3P-memory: SACSegmentation::segment, then optimizeModelCoefficients]: the centroid m = (sum p) / count and S = (sum (p - m)(p - m)^T) / count
 * in fp64, each sum a fixed-order sum over the inliers in ascending input index (blocks of 256 consecutive indices, the library's fixed-order sums);
 * the refined normal is the eigenvector of S's smallest eigenvalue by eig3_sym (cyclic Jacobi), negated if its fp64 dot product with the RANSAC
 * normal is < 0; d = -(n.m); the result rounded to fp32; the inlier set re-selected over the whole cloud with the refined model.  coeff[4] are the
 * fp32 values that selected the reported inliers, widened to double: the rule applied to coeff reproduces the reported set exactly.
 *   Outputs: out_index / out_xyzc follow the outlier filters' rules -- ascending input index, 16-byte records, room for n, each nullable, entries
 * behind *n_out untouched; negative != 0: they receive the complement, the ground-removed cloud that goes straight into rgc_cluster_extract on the
 * device.  *n_out = points written (counted also when both are NULL).  out_counts (nullable, host): one int per stream position the decision used
 * (positions 0 .. info.positions - 1): the count, -1 for an invalid position; untouched behind them.
 *   Refusals: RGC_ERR_INVALID for n < 0, 0 < n < 3, n > 2^27, a threshold not finite or <= 0 (as a float too), probability outside (0, 1),
 * max_iterations < 1, a model_type outside 0..1, and for RGC_PLANE_PERPENDICULAR eps_angle outside [0, pi / 2] or a zero or non-finite axis, a bad
 * stride, n_samples < 0, a NULL context, params, cloud (n > 0), coeff or n_out -- nothing is written.  n = 0: RGC_OK, nothing found, zero
 * coefficients.  A non-finite coordinate: RGC_ERR_NONFINITE, detected on the device by the first walk of the cloud, nothing written.  No valid
 * position in the stream: RGC_OK with n_inliers = 0 and zero coefficients (PCL prints an error); there is no model then, so no point is an inlier and
 * negative != 0 writes the whole cloud.
 *   rgc_plane_set_batch: the positions scored per launch and host round trip (1 .. RGC_PLANE_MAX_BATCH; 0 = automatic: min(max_iterations, 64));
 * NO OUTPUT BIT DEPENDS ON IT.  rgc_plane_get_info: the LAST rgc_plane_segment. */
enum { RGC_PLANE_PLANE = 0, RGC_PLANE_PERPENDICULAR = 1 };
#define RGC_PLANE_MAX_BATCH 1024
typedef struct rgc_plane_params {
  double distance_threshold;  /* PCL's default is 0: it must be set                            */
  double probability;         /* 0.99                                                          */
  double eps_angle;           /* radians; RGC_PLANE_PERPENDICULAR only                         */
  double axis[3];             /* RGC_PLANE_PERPENDICULAR only                                  */
  unsigned long long seed;    /* of the generated stream (no samples)                          */
  int max_iterations;         /* 50                                                            */
  int optimize;               /* 1: setOptimizeCoefficients                                    */
  int model_type;             /* RGC_PLANE_PLANE                                               */
  int reserved;
} rgc_plane_params;
typedef struct rgc_plane_info {
  int n;                      /* points in                                                     */
  int n_inliers;              /* inliers of the reported coefficients                          */
  int iterations;             /* valid positions the decision counted                          */
  int best_count;             /* the best position's count, before refinement (-1: none)       */
  int batch;                  /* positions per launch the call used                            */
  int launches;               /* scoring launches = host round trips of the decision           */
  int refined;                /* 1: the coefficients are the refinement's                      */
  int reserved;
  long long positions;        /* stream positions the decision used (iterations + skipped)     */
  long long skipped;          /* invalid positions among them                                  */
  long long best_position;    /* -1: none                                                      */
  double k;                   /* the final k                                                   */
  double ransac_coeff[4];     /* the best model before refinement (fp32 values widened)        */
} rgc_plane_info;
RGC_API void rgc_default_plane_params(rgc_plane_params* p);
RGC_API int rgc_plane_segment(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, int on_device, const rgc_plane_params* params,
                              const int* samples /* nullable, host, 3 * n_samples */, int n_samples, int negative, double* coeff /* 4, host */,
                              float* out_xyzc /* nullable, n records */, int* out_index /* nullable, n */, int* out_counts /* nullable, host */, int* n_out);
RGC_API int rgc_plane_get_info(rgc_ctx* ctx, rgc_plane_info* info);
RGC_API int rgc_plane_set_batch(rgc_ctx* ctx, int batch);
RGC_API int rgc_plane_sample(unsigned long long seed, unsigned long long t, int n, int* ijk /* 3 */);

/* ---- surface normal estimation: pcl::NormalEstimation, a unit normal and a curvature per point from the second moment of its neighbourhood -- the step a
 * PCL pipeline runs beside the outlier filters, the ground removal and the clustering, and what region growing, SACMODEL_NORMAL_PLANE and point-to-plane
 * terms start from.  (The reference's three nodes do not call the PCL class; rgc_get_target_covariances gives the registration target's normals only,
 * with the solve's k, in fp64 and without a radius, a viewpoint, a curvature or a second cloud to search in.)  Nothing of a neighbour row reaches memory. ----
 *   rgc_normal_estimate -- restated from PCL's features/impl/normal_3d.hpp and features/normal_3d.h FROM MEMORY [3P-memory] (PCL is not available to this
 * project).
 *   Argument rules, on_device and the record format are the outlier filters': x, y, z as floats at the head of each record of its cloud's stride; on_device
 * covers BOTH clouds AND every output (all host memory or all device memory of the context's GPU); n and n_surface <= 2^27.  The call builds a grid of
 * its own over the surface cloud (the search index's machinery and its automatic cell rule): a caller's search index, source and target are untouched.
 * A solve in flight refuses the call (RGC_ERR_INVALID).  rgc_normal_set_cell fixes the grid's cell size for tests and tuning (0 = automatic; finite and
 * >= 0); what depends on it is said under Moments.
 *   Neighbourhood: the neighbours of query i = record i of xyzc come from `surface` (setSearchSurface), or from xyzc itself when surface is NULL
 * (n_surface and surface_stride_bytes are then ignored).  Key: the fp32 ((dx dx + dy dy) + dz dz), never FMA-contracted, as everywhere in this library.
 *   k route (params->k in 3..RGC_NORMAL_MAX_K, radius = 0; setKSearch): the min(k, n_surface) smallest entries in ascending (key, index) -- the search
 * index's total order, so a row is unique whatever ties at its k-th place.  The point itself is a member when the cloud is its own surface, as
 * nearestKSearch returns it.
 *   Radius route (params->radius > 0, k = 0; setRadiusSearch): every surface point with key < r2, STRICT, r2 = (float)((double)radius * (double)radius) --
 * rgc_search_radius' and rgc_outlier_radius' membership rule.  There is no cap on the members.
 *   out_count[i] = m_i, the members used.
 *   Moments: everything is fp64 about the query q.  d_j = (double)P_j - (double)q per axis, S1 = sum d_j, S2 = sum d_j d_j^T (each product rounded, then
 * added), mean = S1 / m, centroid = q + mean, cov = S2 / m - mean mean^T: PCL's computeMeanAndCovarianceMatrix, which normalises by the count m and not
 * by m - 1, with the origin shifted to the query.  k route: ONE chain in ascending rank -- no output bit depends on the grid, the cell size, the launch
 * shape or the run.  Radius route: a fixed order that is a function of the grid and the query alone (every lane of the query's group adds its members in
 * ascending position of the grid's sorted array, the lanes' chains are added in lane order; no floating-point atomic): the bits are identical from run to
 * run and between host-pointer and device-pointer calls, the count m does not depend on the grid, THE LAST BITS OF THE MOMENTS -- and with them of every
 * floating-point output of this route -- MAY DEPEND ON THE CELL SIZE.
 *   Normal: the eigen-decomposition of cov by cyclic Jacobi (the library's eig3_sym); the normal is the column of the smallest eigenvalue, which is the
 * LAST of a descending selection sort of the three eigenvalues, exact ties included (the rule of the registration target's normals), of unit length.
 * curvature = (float)(|lambda_min| / trace), trace = (cov_xx + cov_yy) + cov_zz, when trace > 0, else 0.
 *   Sign: flip = 1 (PCL, flipNormalTowardsViewpoint): the normal is negated when ((vx - qx) nx + (vy - qy) ny) + (vz - qz) nz < 0, evaluated in fp64 in this
 * order, never contracted; an exact 0 keeps the sign the solver gave.  flip = 0: the component of largest magnitude is made positive, the first one
 * on ties.  out_normal4[i] = the fp32 rounding of the fp64 normal, and the curvature.
 *   Too few members: m < 3 gives four quiet NaNs in out_normal4 and NaN rows in out_cov6 / out_centroid, as PCL does (it clears is_dense); out_count still
 * holds m.  *n_valid counts the other queries.
 *   Refusals (RGC_ERR_INVALID, nothing written): both or neither of k / radius set, k outside 3..RGC_NORMAL_MAX_K, radius or r2 not finite or <= 0 (a
 * negative k or radius is out of range), a non-finite viewpoint, flip not 0 / 1, a bad stride, a NULL cloud with n > 0, surface != NULL with n_surface
 * <= 0, a cloud beyond 2^27 points, NULL params / n_valid / context, n < 0.  n = 0: RGC_OK with *n_valid = 0.  A non-finite coordinate in either cloud:
 * RGC_ERR_NONFINITE, detected on the device before the estimate runs, nothing written.  RGC_ERR_GRID_TOO_LARGE as elsewhere.
 *   Deviations from PCL: fp64 moments about the query where PCL sums fp32 unshifted (its result degrades with the distance from the origin; this one
 * does not); the strict radius rule (key < r2) on every route; the tie rule of equal eigenvalues and the sign of an exact 0 (PCL leaves both to Eigen);
 * the flip = 0 sign rule (PCL has none); m < 3 is NaN also on the k route when the surface holds fewer than three points.  Not built: the indices subset
 * (setIndices), the OMP and integral-image variants, PointNormal output packing.
 *   rgc_normal_get_info: the LAST rgc_normal_estimate. */
#define RGC_NORMAL_MAX_K 32
enum { RGC_NORMAL_ROUTE_K = 0, RGC_NORMAL_ROUTE_RADIUS = 1 };
typedef struct rgc_normal_params {
  int k;              /* setKSearch: 3 .. RGC_NORMAL_MAX_K selects the k route, 0 = not this route */
  int flip;           /* 1 (PCL): flipNormalTowardsViewpoint; 0: the written sign rule above       */
  double radius;      /* setRadiusSearch: > 0 selects the radius route; exactly one of k, radius   */
  float viewpoint[3]; /* setViewPoint, default 0 0 0                                               */
  int reserved;
} rgc_normal_params;
typedef struct rgc_normal_info {
  int n, n_surface;      /* queries, surface points (= n when the cloud is its own surface)      */
  int n_valid;           /* queries with three members or more                                   */
  int route;             /* RGC_NORMAL_ROUTE_K / RGC_NORMAL_ROUTE_RADIUS                          */
  double cell;           /* the grid the call used: its cell size                                */
  long long cells;       /* ... and its cells                                                    */
  long long candidates;  /* indexed points looked at over all queries                            */
  int grown;             /* k route: queries whose cube of cells had to grow                     */
  int reserved;
} rgc_normal_info;
RGC_API void rgc_default_normal_params(rgc_normal_params* p); /* k = 0, radius = 0, flip = 1, viewpoint 0 0 0: a caller must choose a route, as in PCL */
RGC_API int rgc_normal_estimate(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, const float* surface /* nullable */, int n_surface,
                                int surface_stride_bytes, int on_device, const rgc_normal_params* params,
                                float* out_normal4 /* nullable, n x (nx, ny, nz, curvature) */, double* out_cov6 /* nullable, n x {xx,xy,xz,yy,yz,zz} */,
                                double* out_centroid /* nullable, n x 3 */, int* out_count /* nullable, n */, int* n_valid);
RGC_API int rgc_normal_get_info(rgc_ctx* ctx, rgc_normal_info* info);
RGC_API int rgc_normal_set_cell(rgc_ctx* ctx, double cell);

/* ---- FPFH descriptors: pcl::FPFHEstimation, a 33-bin Fast Point Feature Histogram per point from the point's neighbourhood and the normals of everything
 * within a radius -- the first consumer of rgc_normal_estimate's normals, the standard descriptor of global registration and place re-recognition, and on
 * the loop-closure path (rgc_kf_detect_loop -> rgc_icp_align) what gives an initial guess that does not depend on the odometry's drift.  (The reference's
 * three nodes do not call the PCL class.)  No neighbour row reaches memory and nothing is looped over on the host. ----
 *   rgc_fpfh_estimate -- restated from PCL's features/impl/fpfh.hpp, features/fpfh.h and features/impl/pfh_tools.hpp (computePairFeatures) FROM MEMORY
 * [3P-memory] (PCL is not available to this project).
 *   Inputs: queries xyzc (n records) and an optional `surface` (setSearchSurface, n_surface records; NULL: xyzc is its own surface, n_surface and
 * surface_stride_bytes are then ignored).  `normals`: one record of three floats (nx, ny, nz at the head of a record of normal_stride_bytes) per SURFACE
 * point -- per xyzc point when surface is NULL.  With a 16-byte stride rgc_normal_estimate's out_normal4 is passed as it is, on the device.  Normals are
 * used as given and are not re-normalised.  Argument rules, on_device and the record format are rgc_normal_estimate's: on_device covers every cloud, the
 * normals AND every output (all host memory or all device memory of the context's GPU); n and n_surface <= 2^27.  The call builds a grid of its own over
 * the surface cloud (the search index's machinery and its automatic cell rule): a caller's search index, source and target are untouched.
 * A solve in flight refuses the call (RGC_ERR_INVALID).  rgc_fpfh_set_cell fixes the grid's cell size for tests and tuning (0 = automatic; finite and
 * >= 0).
 *   Rows: the radius route only.  params->radius > 0, r2 = (float)((double)radius * (double)radius).  Surface point j is a member of the row of point p
 * when the library's fp32 key ((dx dx + dy dy) + dz dz), never FMA-contracted, is < r2, STRICT.  m_p is the row size; it includes p itself when p is a
 * surface point.
 *   Valid surface point: its three normal components are finite.  A non-finite COORDINATE in either cloud is RGC_ERR_NONFINITE, as elsewhere, detected
 * on the device before anything is written; a non-finite NORMAL is data (rgc_normal_estimate emits NaN rows).
 *   Pair term of a valid surface point s (normal a) with row member t (normal b), everything in fp64 from the fp32 inputs, every product rounded and
 * then added, never contracted.  The pair is skipped if the fp32 key is 0 or t is not valid.  d = t - s per axis; f4 = sqrt((dx dx + dy dy) + dz dz);
 * c1 = (ax dx + ay dy) + az dz, c2 likewise with b.  Swap iff |c1| < |c2|, strict: the decision is on the numerators, not on quotients or acos.  If
 * swapped u = b, n2 = a, d = -d, f3 = -c2 / f4; otherwise u = a, n2 = b, f3 = c1 / f4.  v = d x u, vn = sqrt((vx vx + vy vy) + vz vz); the pair is
 * skipped if vn == 0; v /= vn per component.  w = u x v.  f2 = (vx n2x + vy n2y) + vz n2z.  f1 = atan2((wx n2x + wy n2y) + wz n2z, (ux n2x + uy n2y) +
 * uz n2z).  Bins, each clamped to 0..10: b1 = floor(11 ((f1 + pi) (1 / (2 pi)))), b2 = floor(11 ((f2 + 1) 0.5)), b3 = floor(11 ((f3 + 1) 0.5)).
 *   SPFH of s: three blocks of 11 INTEGER counts of its non-skipped pairs (bins b1, 11 + b2, 22 + b3), plus m_s; skipped pairs still count in m_s.  As
 * numbers SPFH_s[b] = count inc_s, inc_s = 100.0 / (double)(m_s - 1); every entry is zero when m_s <= 1 or s is not valid.  The counts are exact: no bit
 * depends on the order, the grid, the cell size or the launch.  out_spfh (n_surface x 33, nullable) and out_spfh_count (n_surface, nullable; n rows when
 * surface is NULL) read them out: out_spfh_count holds m_s, and -1 (with a row of zeros) where the SPFH was not computed.
 *   Which SPFHs are computed: with surface == NULL every point's; with a separate surface only those of surface points that are a member of some
 * query's row (a mark pass over the queries, a compaction, then the SPFH pass over the marked points).  info.n_spfh reports how many: a function of the
 * inputs alone.
 *   FPFH of query q: over its row members j with key > 0 and j valid, w_j = 1.0 / (double)key_j, F[b] = sum_j ((double)count_j[b] inc_j) w_j.  As in PCL
 * the query's own SPFH is not part of its FPFH, and the query's own normal is never read.  Per block of 11, sum = F[0] + ... + F[10] in ascending bin;
 * if sum != 0, out[b] = (float)(F[b] (100.0 / sum)), otherwise the block is 0.  Summation order: as on the normals' radius route a fixed function of
 * the grid and the query alone -- ONE chain per bin, the members added in the order the query's walk over the grid meets them (layer by layer, row by
 * row of cells, ascending position in the grid's sorted array); no floating-point atomic: the bits are identical from run to run and between
 * host-pointer and device-pointer calls, the counts do not depend on the grid, THE LAST BITS OF out_fpfh MAY DEPEND ON THE CELL SIZE.
 * out_count[i] = m_q.  m_q == 0 (possible only with a separate surface) gives 33 quiet NaNs; *n_valid counts the other queries.
 *   Refusals (RGC_ERR_INVALID, nothing written): radius or r2 not finite or <= 0, a bad stride (a cloud's or the normals': < 12, not a multiple of 4 or
 * > 4096), a NULL cloud or NULL normals with n > 0, surface != NULL with n_surface <= 0, a cloud beyond 2^27 points, NULL params / n_valid / context,
 * n < 0.  n = 0: RGC_OK with *n_valid = 0.  RGC_ERR_GRID_TOO_LARGE as elsewhere.
 *   Deviations from PCL: fp64 pair terms where PCL uses fp32; the swap test on the numerators where PCL compares acosf values; the strict radius rule
 * (key < r2); invalid normals skipped pair by pair where PCL propagates NaN or requires a dense cloud.  Not built: the k route, the indices subset
 * (setIndices), setNrSubdivisions other than 11 / 11 / 11, FPFHEstimationOMP, descriptor matching and the SAC-IA / prerejective alignment on top.
 *   rgc_fpfh_get_info: the LAST rgc_fpfh_estimate. */
#define RGC_FPFH_BINS 33
typedef struct rgc_fpfh_params {
  double radius;   /* setRadiusSearch: > 0; the default 0 is refused -- a caller must choose */
  int reserved[2];
} rgc_fpfh_params;
typedef struct rgc_fpfh_info {
  int n, n_surface;      /* queries, surface points (= n when the cloud is its own surface)      */
  int n_valid;           /* queries with at least one member                                     */
  int n_spfh;            /* surface points whose SPFH was computed                               */
  double cell;           /* the grid the call used: its cell size                                */
  long long cells;       /* ... and its cells                                                    */
  long long pairs;       /* non-skipped pair terms                                               */
  long long candidates;  /* indexed points looked at over all passes                             */
  int reserved[2];
} rgc_fpfh_info;
RGC_API void rgc_default_fpfh_params(rgc_fpfh_params* p); /* radius = 0: a caller must choose */
RGC_API int rgc_fpfh_estimate(rgc_ctx* ctx, const float* xyzc, int n, int stride_bytes, const float* surface /* nullable */, int n_surface,
                              int surface_stride_bytes, const float* normals, int normal_stride_bytes, int on_device, const rgc_fpfh_params* params,
                              float* out_fpfh /* nullable, n x 33 */, unsigned* out_spfh /* nullable, n_surface x 33 */,
                              int* out_spfh_count /* nullable, n_surface */, int* out_count /* nullable, n */, int* n_valid);
RGC_API int rgc_fpfh_get_info(rgc_ctx* ctx, rgc_fpfh_info* info);
RGC_API int rgc_fpfh_set_cell(rgc_ctx* ctx, double cell);

/* ---- in-library kernel timing with HIP events on the context's stream (bench.py roofline) ---- */
enum {
  RGC_K_GRID = 0,      /* bbox + count + scan + scatter + rank/gather                         */
  RGC_K_KNN_COV = 1,   /* exact kNN + covariance + normal, bulk kernel on the TARGET (dominant) */
  RGC_K_VOXEL = 2,     /* Gaussian voxel map reduction                                        */
  RGC_K_LINEARIZE = 3, /* correspondences + Mahalanobis + H/b/cost                            */
  RGC_K_ERROR = 4,     /* frozen-correspondence cost                                          */
  RGC_K_FITNESS = 5,   /* 1-NN fitness                                                        */
  RGC_K_KNN_COV_SRC = 6, /* the same kernel on the (small) source cloud, separate instantiation */
  RGC_K_KNN_COOP = 7,    /* cooperative kernel (one wave per deferred query), target               */
  RGC_K_KNN_COOP_SRC = 8,/* cooperative kernel, source                                             */
  RGC_K_COUNT = 9
};
RGC_API int rgc_profile_enable(rgc_ctx* ctx, int on);
/* restrict the event regions to the kinds whose bit is set (bit k = kind k; default: all).  Each region costs two
 * hipEventRecord calls, so a timed run that only needs one kernel's duration selects just that kind. */
RGC_API int rgc_profile_select(rgc_ctx* ctx, unsigned kind_mask);
RGC_API int rgc_profile_reset(rgc_ctx* ctx);
/* launches = timed regions of that kind; total_ms = summed hipEventElapsedTime; last_n = points of the last region */
RGC_API int rgc_profile_get(rgc_ctx* ctx, int kind, long long* launches, double* total_ms, long long* total_points);
RGC_API const char* rgc_profile_name(int kind);

#ifdef __cplusplus
}
#endif
#endif /* RGC_HIP_H */
