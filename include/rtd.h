/*
 * rtd.h — C ABI of the MI355X pencil-beam proton dose engine.
 *
 * This is the drop-in boundary for the reference's single hot-path entry point
 *
 *     void cudaWrapperProtons(HostPinnedImage3D<float>* imVol, HostPinnedImage3D<float>* doseVol,
 *                             const std::vector<BeamSettings> beams, const EnergyStruct iddData,
 *                             std::ostream& outStream);            (reference src/kernel_wrapper.cuh:161)
 *
 * Every struct below is the plain-C image of one reference host type; every function cites the
 * part of the reference it replaces. No C++/STL/torch types cross this boundary: plain pointers,
 * sizes and PODs only. All arrays are x-fastest ("[z][y][x]"), float32, exactly as in the reference.
 *
 * Threading: one handle per host thread; a handle owns one HIP device, one stream and all device
 * memory it allocates. Functions return RTD_OK (0) or a negative rtd_status; rtd_last_error()
 * returns the message (the reference throws std::runtime_error / const char* instead,
 * src/cuda_errchk.cu:11-22, src/kernel_wrapper.cu:965).
 */
#ifndef RTD_H
#define RTD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTD_ABI_VERSION 3

typedef enum rtd_status {
    RTD_OK = 0,
    RTD_ERR_INVALID_ARG = -1,     /* null pointer, zero dimension, empty energy list (vector_find.h:24) */
    RTD_ERR_HIP = -2,             /* a HIP runtime call or kernel launch failed (cuda_errchk.cu:11-22) */
    RTD_ERR_RADIUS_OVERFLOW = -3, /* "Found larger than allowed kernel superposition radius" (kernel_wrapper.cu:965) */
    RTD_ERR_NOT_READY = -4,       /* CT or LUTs not set before compute */
    RTD_ERR_IO = -5,              /* LUT directory unreadable (energy_reader.cpp:21-24) */
    RTD_ERR_NO_DEVICE = -6        /* no HIP device: the engine has no CPU fallback */
} rtd_status;

/* Float3AffineTransform (src/float3_affine_transform.cuh): y = M x + v, M row-major. */
typedef struct rtd_affine {
    float m[9];
    float v[3];
} rtd_affine;

/* Float3IdxTransform (src/float3_idx_transform.cuh): y = x*delta + offset, component-wise. */
typedef struct rtd_idx_transform {
    float delta[3];
    float offset[3];
} rtd_idx_transform;

/*
 * BeamSettings (src/beam_settings.h:101-109), all nine fields.
 * spot_weights: [n_layers][spot_ny][spot_nx] particle numbers (beam_settings.h:21). Caller-owned; the
 * engine never frees it (the reference deletes it, kernel_wrapper.cu:856 — the C++ shim can mimic that).
 */
typedef struct rtd_beam {
    const float* spot_weights;
    uint32_t spot_nx, spot_ny, n_layers;
    const float* energies;            /* [n_layers] MeV/u */
    const float* spot_sigmas;         /* [n_layers][2] (sigma_x, sigma_y) mm at iso in air */
    float ray_spacing[2];             /* mm between adjacent rays at iso */
    uint32_t tracer_steps;            /* number of ray-trace steps */
    float source_dist[2];             /* apparent source-to-iso distance in x and y, mm; may be +inf */
    rtd_idx_transform spot_idx_to_gantry; /* delta.z = (negative) step length, offset.z = start depth */
    rtd_affine gantry_to_im_idx;      /* gantry mm -> CT voxel index */
    rtd_affine gantry_to_dose_idx;    /* gantry mm -> dose voxel index */
} rtd_beam;

/* EnergyStruct (src/energy_struct.h:13-31). cidd_matrix is [n_energies][n_energy_samples]. */
typedef struct rtd_luts {
    int32_t n_energy_samples;
    int32_t n_energies;
    const float* energies_per_u;   /* [n_energies] ascending */
    const float* peak_depths;      /* [n_energies] mm */
    const float* scale_facts;      /* [n_energies] samples per mm */
    const float* cidd_matrix;      /* [n_energies*n_energy_samples] cumulative IDD */
    int32_t n_density_samples;
    float density_scale_fact;
    const float* density_vector;   /* mass density vs (HU+1000)*scale */
    int32_t n_sp_samples;
    float sp_scale_fact;
    const float* sp_vector;        /* relative stopping power vs (HU+1000)*scale */
    int32_t n_rrl_samples;
    float rrl_scale_fact;
    const float* rrl_vector;       /* 1/X0 per unit density vs density*scale */
    /* NUCLEAR_CORR only (energy_struct.h:33-36, energy_reader.cpp:103-162); may be NULL when options.nuclear_corr == 0 */
    const float* nuc_weight_matrix;   /* [n_energies*n_energy_samples] fraction of the dose in the nuclear halo        */
    const float* nuc_sq_sigma_matrix; /* [n_energies*n_energy_samples] squared sigma of the halo, mm^2                  */
} rtd_luts;

/*
 * The reference's compile-time physics switches (CMakeLists.txt:36-79) as run-time options.
 * rtd_default_options() returns the reference defaults.
 */
typedef struct rtd_options {
    int32_t dose_to_water;      /* DOSE_TO_WATER (ON)  kernel_wrapper.cu:314-318 */
    int32_t nozzle;             /* NOZZLE (ON); 0 = NO_NOZZLE  fill_idd_and_sigma_params.cu:74-83 */
    float bp_depth_cutoff;      /* BP_DEPTH_CUTOFF   1.05 */
    float conv_sigma_cutoff;    /* CONV_SIGMA_CUTOFF 3.0  */
    float ks_sigma_cutoff;      /* KS_SIGMA_CUTOFF   3.0  */
    float ray_weight_cutoff;    /* RAY_WEIGHT_CUTOFF 1.0  */
    int32_t fine_grained_timing;/* FINE_GRAINED_TIMING: per-stage hipEvent buckets */
    int32_t nuclear_corr;       /* NUCLEAR_CORR (OFF): RTD_NUC_* below. CMakeLists.txt:57-69                             */
    int32_t reserved[3];
} rtd_options;

/*
 * NUCLEAR_CORR: a second, broad Gaussian per spot (the nuclear halo) on a grid at spot resolution. The reference ships this
 * path switched OFF and unfinished: the constants of the variants carry the comment "CORRECT ALL THESE"
 * (kernel_wrapper.cu:230), and the fill kernel is constructed with a nuclear memory step of 0 (:925, 7th argument), so every
 * step of a ray overwrites the SAME nuclear voxel (:367-373) and the halo reaches the dose only through BEV slice 0, i.e. only
 * when the beam starts inside the patient. This engine restates what that code does, quirk included (the primary dose loses the
 * nuclear fraction; the halo deposit is whatever slice 0 receives); it does not repair it.
 */
enum { RTD_NUC_OFF = 0, RTD_NUC_SOUKUP = 1, RTD_NUC_FLUKA = 2, RTD_NUC_GAUSS_FIT = 3 };

/*
 * Per-field timing record; bucket names follow the reference's FINE_GRAINED_TIMING printout
 * (kernel_wrapper.cu:1298-1307). All values in milliseconds, measured with hipEvents on the
 * handle's stream. Only filled when options.fine_grained_timing != 0 (else total_ms only).
 */
typedef struct rtd_timing {
    float raytracing_ms;          /* "Time to trace ... rays"                    */
    float prepare_energy_loop_ms; /* plan + BEV zero + spot->ray convolution     */
    float fill_idd_sigma_ms;      /* "Time depositing IDD and calculating sigma" */
    float prepare_superp_ms;      /* tile radius classification + batching       */
    float superp_ms;              /* "Time executing superposition"              */
    float transforming_ms;        /* "Kernel time to transform ... voxels"       */
    float total_ms;               /* first kernel to last kernel of the field    */
    int32_t superp_launches;      /* number of superposition kernel launches     */
    float superp_kernel_ms;       /* the dominant kernel alone (k_superpose_mfma), inside superp_ms */
    uint32_t ray_dims[2];         /* what the reference's timing lines quote: "trace WxH rays S steps", "N time(s)" per   */
    uint32_t steps;               /* layer, "transform N voxels" (kernel_wrapper.cu:1298-1307)                           */
    uint32_t n_layers;
    int64_t transfer_voxels;      /* voxels of the dose box the transfer visited */
    int32_t reserved[2];
} rtd_timing;

/* Geometry and cut-off scalars of the last computed field (for logs, tests and the roofline model). */
typedef struct rtd_field_info {
    uint32_t ray_dims[3];         /* primRayDims (W, H, L)  kernel_wrapper.cu:659 */
    float ray_offset[3];          /* primRayOffset          kernel_wrapper.cu:654 */
    float ray_res[3];             /* primRayRes             kernel_wrapper.cu:623 */
    int32_t beam_first_inside;    /* kernel_wrapper.cu:781-784 */
    int32_t beam_first_outside;   /* kernel_wrapper.cu:785-787 */
    int32_t beam_first_guaranteed_passive; /* kernel_wrapper.cu:796 */
    int32_t beam_first_calculated_passive; /* kernel_wrapper.cu:955-957 */
    int32_t bbox_min[3];          /* kernel_wrapper.cu:1207 */
    int32_t bbox_max[3];          /* kernel_wrapper.cu:1208 */
    int64_t live_steps;           /* sum over layers of (layerFirstPassive - beamFirstInside) */
    int32_t max_radius;           /* largest tile radius over all layers */
    int32_t dose_box_min[3];      /* sub-box of bbox that this field can have changed: the image of the BEV rectangle that */
    int32_t dose_box_max[3];      /* carries dose (what rtd_field_clear_dose clears; what has to cross PCIe); with nuclear_corr
                                     the whole grid (the halo's own box is wider and known on the device only)             */
    int32_t uniform_sigma;        /* 1: every (layer, step) slice had one sigma over its live rays (a water phantom) and the
                                     superposition ran as a separable convolution (k_superpose_uniform); decided on the device */
} rtd_field_info;

typedef struct rtd_handle_s* rtd_handle;
typedef struct rtd_field_s* rtd_field;

uint32_t rtd_abi_version(void);
void rtd_default_options(rtd_options* out);

/* Replaces cudaFree(0) context init (kernel_wrapper.cu:388); --gpu_id is finally honoured (config.cpp:13-15). */
int rtd_create(int device_id, rtd_handle* out);
int rtd_destroy(rtd_handle h);
const char* rtd_last_error(rtd_handle h);
/* Message for a failure that happened before a handle existed (rtd_create). */
const char* rtd_global_error(void);

int rtd_set_options(rtd_handle h, const rtd_options* opt);

/* LUT upload, replaces the texture set-up (kernel_wrapper.cu:453-537). Arrays are copied. */
int rtd_set_luts(rtd_handle h, const rtd_luts* luts);
/* Reads the reference's LUT text layout from a directory (energy_reader.cpp:12-101) and uploads it.
 * water_cube_test != 0 selects radiation_length_inc_water.txt (energy_reader.cpp:77-93). With options.nuclear_corr set (before
 * this call) the variant's nuclear_weights_and_sigmas_*.txt is read and checked against the IDD table too (:103-162). */
int rtd_load_luts_dir(rtd_handle h, const char* dir, int water_cube_test);

/* CT upload, replaces cudaMemcpy3D into the 3-D texture (kernel_wrapper.cu:420-451).
 * hu_plus_1000: [dims[2]][dims[1]][dims[0]] float, host memory. */
int rtd_set_ct(rtd_handle h, const float* hu_plus_1000, const uint32_t dims[3]);
/* rtd_set_ct without the copy: hu_plus_1000 stays with the caller — valid and unchanged until the last compute that uses it has
 * been finished — and every field uploads, in front of its tracer, only the index box of the volume its rays can sample (a beam
 * of the 512^3 bench plan reads a tenth of the CT; the upload of all 537 MB was 9.4 of the 13 ms of a one-field call). */
int rtd_set_ct_deferred(rtd_handle h, const float* hu_plus_1000, const uint32_t dims[3]);
/* Same, for a CT already resident on this handle's device (not copied, not owned).
 * A BOUND VOLUME IS ANNOUNCED AS CHANGED BY CALLING rtd_set_ct* AGAIN (rtd_set_ct_device with the same pointer, rtd_set_ct_deferred
 * with the same host volume): the handle cannot see a volume rewritten in place, and a field keeps between computes what it
 * derived from CT, LUTs and options (see rtd_field_compute below). Every rtd_set_ct*, rtd_set_luts, rtd_load_luts_dir and
 * rtd_set_options call makes every field of the handle derive it again at its next compute. */
int rtd_set_ct_device(rtd_handle h, const float* dev_hu_plus_1000, const uint32_t dims[3]);

/*
 * The reference-shaped call: for every beam run the whole path and ACCUMULATE into dose_inout
 * (host memory, [dims[2]][dims[1]][dims[0]]): upload dose (kernel_wrapper.cu:542), beam loop (:601-1312),
 * download (:1318). timing may be NULL; else it must point to n_beams records.
 */
int rtd_compute(rtd_handle h, const rtd_beam* beams, int n_beams, float* dose_inout,
                const uint32_t dose_dims[3], rtd_timing* timing);

/*
 * Split form for callers that keep data resident (benchmarks, multi-GPU plans):
 * rtd_field_create   host geometry + workspace allocation + spot-weight upload for one beam
 *                    (kernel_wrapper.cu:612-734, 851-852);
 * rtd_field_compute  launches every kernel of the field on the handle's stream and accumulates into
 *                    dev_dose (device memory of this handle's device). Asynchronous: no host sync,
 *                    no allocation, so it can be captured into a hipGraph;
 * rtd_field_finish   waits for the field's last launch (not for later work on the stream) and reports device-side
 *                    errors (radius overflow), timing and geometry of that launch;
 * rtd_field_clear_dose  zeroes, on the stream, exactly the voxels of dev_dose that the field's last
 *                    rtd_field_compute could have changed (its device-side dose box). A plan loop that starts
 *                    every iteration from an all-zero volume (the reference uploads a zero dose image per call,
 *                    main.cu:192-206, kernel_wrapper.cu:542) restores it with this instead of clearing all of it.
 *
 * What a field keeps between computes: its ray trace (density, WEPL, radiation length, entry and exit steps) and the plan made
 * from it (cut-off steps, entry plane and entry sigmas), which depend on CT, LUTs, options and the beam's geometry but not on the
 * spot weights. Once a compute of the field has been FINISHED (rtd_field_finish, rtd_field_wait_plan, rtd_field_dose_influence)
 * without a device-side error, a later rtd_field_compute / _compute_bev with no rtd_set_ct*, LUT or options call in between
 * launches neither the tracer nor the plan (with a deferred CT it uploads nothing either); the result is bit for bit that of a full
 * compute. rtd_field_set_spot_weights keeps the trace, so the re-weighting loop of an optimiser traces once; a CT rewritten in
 * place must be announced (rtd_set_ct_device above). Not kept: across rtd_field_release; with nuclear_corr; for spot maps of more
 * than 64 rows; by launches into a capturing stream (a graph holds the full sequence). rtd_timing of such a compute: raytracing_ms
 * = 0, total_ms from its first launch. rtd_field_fetch "trace_reused" tells which kind the last launched compute was.
 *
 * With the trace a field keeps a sigma record: what the fill's sigma recurrence gives for every (layer, step, ray) when the spot
 * weights are left out of it (a ray below ray_weight_cutoff is masked afterwards). The first compute that reuses the trace records
 * it in front of its fill (inside fill_idd_sigma_ms) and replays it; the computes after a finished such compute replay it under
 * their own weights, bit for bit the result of the recurrence. Same validity as the trace (kept by rtd_field_set_spot_weights and by
 * the batches of rtd_field_dose_influence; dropped by rtd_set_ct*, LUT and options calls and by rtd_field_release; never with
 * nuclear_corr, spot maps of more than 64 rows, or in a capturing stream). Memory per field, allocated by that first compute: 4
 * bytes x layers x rays x (steps from the entry step to the last step a layer can reach) + 4 bytes x layers x rays, about 135 MB on
 * a 96 x 88 x 20 ray grid with 200 such steps; if the allocation fails the field keeps computing the recurrence and no error is
 * raised. RTD_NO_SIGMA_REUSE in the environment when the field is created: every compute runs the recurrence.
 * rtd_field_fetch "sigma_reused" tells what the last launched compute did.
 *
 * Beside the sigma record a field whose fill fits the GPU at once — 2 x layers x (ray grid / 256) blocks of 256 threads all
 * resident: about 1800 blocks on an MI355X; larger fields keep none and compute their dose as before — keeps a dose record of the
 * same extent (as many bytes again, so budget twice the figure above for such a field): per (layer, step, ray) the
 * difference of the cumulative depth dose that the fill's dose walk looks up, or a mark where the walk forces the dose to 0. It is
 * allocated, recorded, valid and dropped with the sigma record, and the replay forms the dose from it with the walk's own operations:
 * bit for bit the walk's result. If its allocation alone fails the field replays sigma and walks the dose; no error is raised.
 * RTD_NO_DOSE_REPLAY in the environment when the field is created: no dose record (RTD_NO_SIGMA_REUSE and RTD_NO_TRACE_REUSE leave
 * it out too). rtd_field_fetch "dose_reused" tells what the last launched compute did. A compute that records or replays both
 * records checks that every step of every layer lies inside them; if not (the inputs were changed in place without rtd_set_ct*),
 * rtd_field_finish, rtd_field_wait_plan and rtd_field_dose_influence return RTD_ERR_NOT_READY, the records and the trace are
 * dropped, and the next compute traces and walks again.
 */
int rtd_field_create(rtd_handle h, const rtd_beam* beam, const uint32_t dose_dims[3], rtd_field* out);
int rtd_field_compute(rtd_handle h, rtd_field f, float* dev_dose);
int rtd_field_finish(rtd_handle h, rtd_field f, rtd_timing* timing, rtd_field_info* info);
int rtd_field_clear_dose(rtd_handle h, rtd_field f, float* dev_dose);
int rtd_field_destroy(rtd_handle h, rtd_field f);
/* Like rtd_field_destroy, but the device workspace stays with the handle and is taken over by the next rtd_field_create of
 * the same shape (ray grid, steps, layers, spot map): a plan of similar beams allocates once, where the reference mallocs and
 * frees ~20 buffers per beam (kernel_wrapper.cu:685-734, 1265-1281). rtd_compute uses it between its beams. */
int rtd_field_release(rtd_handle h, rtd_field f);

/*
 * The two halves of rtd_field_compute, and the pieces a multi-GPU plan is made of. The beam loop of the reference
 * (kernel_wrapper.cu:601) shares nothing between beams but the final `+=` into the dose volume (:92), so fields shard one
 * per GPU; what then has to cross the xGMI links is NOT the dose: the beam's-eye-view (BEV) dose of a field — the cube the
 * reference copies into a 3-D texture before primTransfDiv samples it (:1107-1141) — is ~10 MB where the dose box it
 * turns into is 60-83 MB (512^3 grid). So a field's BEV slab travels, and every GPU runs the transfer of EVERY field into its
 * own slab of the dose volume:
 * rtd_field_compute_bev   all kernels up to the BEV dose (:766-1105); asynchronous;
 * rtd_field_transfer      fan -> dose-grid transfer (primTransfDiv, :69-97) of the field's BEV dose into dev_dose, restricted
 *                         to the inclusive dose-index box [clip_min, clip_max] (NULL = the whole grid); asynchronous; may be
 *                         called several times (several volumes / boxes) for one BEV dose;
 * rtd_field_wait_plan     waits until the field's device-side plan is known (entry / passive steps, BEV rectangle, dose
 *                         box) — the superposition may still be running — and returns the size of the message below;
 * rtd_field_export_bev    packs [state record | non-zero block of the BEV dose] into dev_buf (device memory, capacity
 *                         bytes; rtd_bev_message_bound() is always enough); asynchronous, after rtd_field_compute_bev;
 * rtd_field_create_remote a field object for a beam computed on ANOTHER GPU: host geometry only, no workspace
 *                         (needs neither LUTs nor CT on this handle);
 * rtd_field_attach_bev    the remote field samples the message at dev_buf (device memory of this handle's device, not
 *                         copied: it must stay valid until the transfers that use it have run); then rtd_field_transfer,
 *                         rtd_field_clear_dose_box and rtd_field_finish work on it as on a local field.
 * rtd_field_clear_dose_box zeroes the part of the field's dose box inside [clip_min, clip_max].
 */
int rtd_field_compute_bev(rtd_handle h, rtd_field f);
int rtd_field_transfer(rtd_handle h, rtd_field f, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]);
/* rtd_field_transfer for the FIRST field of a plan, into a volume that is zero everywhere except possibly inside this
 * field's dose box (e.g. the volume the same field was transferred into by the previous plan): the box is written — dose
 * or zero — instead of accumulated into, which replaces rtd_field_clear_dose + the read half of the read-modify-write. */
int rtd_field_transfer_init(rtd_handle h, rtd_field f, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]);
/* Several fields — own BEV doses and / or attached slabs — into ONE box of the dose grid in one launch: every voxel of the
 * inclusive box [box_min, box_max] (NULL = the whole grid) is WRITTEN with 0 + field 0 + field 1 + ..., the positive samples
 * in list order: bit for bit what rtd_field_transfer of each field in turn accumulates into a zeroed box (the beam loop of
 * kernel_wrapper.cu:601 with its primTransfDiv launches, :1216), without the read-modify-write passes and without a clear.
 * Voxels outside the box are not touched: a GPU of a multi-GPU plan passes its slab of the volume, cut to the bounding box of
 * the fields' dose boxes. At most 16 fields; not with nuclear_corr. rtd_field_finish of the LAST own field of the list (the
 * first field if all are remote) waits for the launch and reports its duration as transforming_ms. */
int rtd_fields_transfer_init(rtd_handle h, const rtd_field* fields, uint32_t n_fields, float* dev_dose, const int32_t box_min[3],
                             const int32_t box_max[3]);
int rtd_field_wait_plan(rtd_handle h, rtd_field f, rtd_field_info* info, size_t* packed_bytes);
size_t rtd_bev_message_bound(rtd_handle h, rtd_field f);
int rtd_field_export_bev(rtd_handle h, rtd_field f, void* dev_buf, size_t capacity);
int rtd_field_create_remote(rtd_handle h, const rtd_beam* beam, const uint32_t dose_dims[3], rtd_field* out);
int rtd_field_attach_bev(rtd_handle h, rtd_field remote_field, const void* dev_buf);
int rtd_field_clear_dose_box(rtd_handle h, rtd_field f, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]);

/* Page-locks / unlocks a caller-owned host buffer so that rtd_set_ct / rtd_compute copy at full PCIe rate — what
 * HostPinnedImage3D's constructor and destructor do with cudaHostRegister (host_image_3d.cuh:23-32, 45-48). */
int rtd_host_register(void* host_ptr, size_t bytes);
int rtd_host_unregister(void* host_ptr);

/* Device buffers owned by the handle (so a C caller needs no HIP headers). */
int rtd_device_alloc(rtd_handle h, size_t bytes, void** dev_ptr);
int rtd_device_free(rtd_handle h, void* dev_ptr);
int rtd_device_zero(rtd_handle h, void* dev_ptr, size_t bytes);
int rtd_copy_to_device(rtd_handle h, void* dev_dst, const void* host_src, size_t bytes);
int rtd_copy_to_host(rtd_handle h, void* host_dst, const void* dev_src, size_t bytes);
int rtd_sync(rtd_handle h);
/* The hipStream_t the handle launches on (as void*), for event timing by the caller. */
void* rtd_stream(rtd_handle h);
/* Use an externally created hipStream_t (e.g. torch's current stream); NULL restores the handle's own. */
int rtd_set_stream(rtd_handle h, void* hip_stream);

/*
 * Introspection for parity tests: copy a named intermediate of the last rtd_field_compute to host.
 * Names: "density" "wepl" [S][H][W] float; "first_inside" "first_outside" [H][W] int32;
 * "wepl_min" [S] float; "ray_weights" [L][H][W] float; "idd" "rsigma" [L][S][H][W] float;
 * "first_passive" [L][H][W] int32; "tile_radius" [L][S][tilesY][tilesX] uint8 (0xFF = not classified);
 * "eff_radius" [L][34] int32 (batch radius per tile radius); "bev" [S][H+64][W+64] float;
 * "layer_plan" [L][8] float (energyIdx, scaleFact, peakDepth, entrySigmaX, entrySigmaY, afterLast, 0, 0);
 * "trace_reused" int32[1]: 1 if the last launched compute reused the field's trace and plan (see rtd_field_compute).
 * "sigma_reused" int32[1]: the sigma recurrence of the last launched compute: 0 walked, 1 recorded and replayed, 2 replayed.
 * "dose_reused" int32[1]: the dose walk of the last launched compute, likewise (never ahead of "sigma_reused").
 * "launch_builds" int32[4]: which kernel builds the field's last launched tracer and fill were (a host record; -1 before the first):
 *   [0] the tracer's sampling kernel after the LDS fallbacks: 0 plain, 1 along-beam, 2 diagonal;
 *   [1] 1 if the fill staged the layer's cumulative-IDD rows in LDS, 0 if it read them from global memory (or looked none up);
 *   [2] the fill's mode: 0 walked, 1 sigma replayed and dose walked, 2 both replayed;
 *   [3] 1 for the NUCLEAR_CORR build of the fill.
 * "target_bev" and "target_hit": see rtd_field_project_target below.
 * Returns the number of bytes the buffer holds via *bytes_needed when host_out is NULL.
 */
int rtd_field_fetch(rtd_handle h, rtd_field f, const char* name, void* host_out, size_t bytes,
                    size_t* bytes_needed);

/*
 * ---- Spot-weight gradients (the transposed dose path) ----
 *
 * For a field whose last rtd_field_compute or rtd_field_compute_bev ran at spot weights w ([L][ny][nx]) and a voxel-weight volume
 * g on the dose grid ([dims[2]][dims[1]][dims[0]] float):
 *
 *     grad[l][sy][sx] = sum_v g[v] * dD[v] / dw[l][sy][sx]
 *
 * D is the dose this field adds to the volume. The set of live rays is frozen at w: a ray is dead when its weight is below
 * ray_weight_cutoff or when it leaves the patient before its layer's first step (afterLast < pFirst, k_fill); dead rays contribute
 * 0. On that live set D is linear for w >= 0, so the result is exact: for every delta >= 0 that keeps the live set,
 * <D(w + delta) - D(w), g> = <delta, grad>. Rays of weight 0 are live under ray_weight_cutoff = 0, and their gradient includes the
 * voxels their dose would reach. Optimisers should set ray_weight_cutoff = 0: with the default cut-off of 1 a spot whose rays all
 * sit below it gets a gradient of 0.
 *
 * rtd_field_spot_gradient  dev_voxel_weights, dev_spot_grad: device memory of this handle's device. WRITES (does not accumulate)
 *                          [L][ny][nx] into dev_spot_grad. Waits for the field's plan (host sync, as rtd_field_wait_plan), then runs
 *                          asynchronously on the handle's stream. Bitwise reproducible; changes neither the field's BEV dose nor
 *                          anything a later transfer reads. The workspace (grad_bev, grad_ray_weights) is allocated by the first call
 *                          and reused. RTD_ERR_NOT_READY before any compute of the field; RTD_ERR_INVALID_ARG for a remote field,
 *                          nuclear_corr or a null pointer; RTD_ERR_RADIUS_OVERFLOW when the forward found one (as rtd_field_finish).
 * rtd_spot_gradient        the host-memory, reference-shaped form: every beam is computed up to its BEV dose and its gradient taken;
 *                          spot_grad_out receives the per-beam [L][ny][nx] blocks concatenated in beam order.
 * rtd_field_fetch names of the last gradient call: "grad_bev" [S][H+64][W+64] float (<g, D> = <grad_bev, bev>) and
 * "grad_ray_weights" [L][H][W] float (<grad_bev, bev> = <grad_ray_weights, ray_weights>).
 * Not available: nuclear_corr, remote fields, the multi-GPU rtd_plan_* path.
 */
int rtd_field_spot_gradient(rtd_handle h, rtd_field f, const float* dev_voxel_weights, float* dev_spot_grad);
int rtd_spot_gradient(rtd_handle h, const rtd_beam* beams, int n_beams, const float* voxel_weights, const uint32_t dose_dims[3],
                      float* spot_grad_out);

/*
 * ---- Dose-influence matrix (Dij): per-spot sparse dose columns of a field ----
 *
 * Dij belongs to a local field, on that field's dose grid, under the options the field was created with. Column j is spot
 * j = (l * ny + sy) * nx + sx, in the [L][ny][nx] order of spot_weights and of rtd_field_spot_gradient; row v is the linear voxel
 * index of the dose grid (x fastest), as int32. Column j is the dose the field adds to the volume when spot j has weight 1 and every
 * other spot weight 0. So Dij w = D(w) (rtd_field_compute) and Dij^T g = rtd_field_spot_gradient(g).
 *
 * options.ray_weight_cutoff must be 0 (else RTD_ERR_INVALID_ARG): only then is the forward linear in the spot weights with a live set
 * that does not depend on them. rel_threshold in [0, 1): entry v of column j is kept iff value != 0 and value >= rel_threshold *
 * max(column j); with 0 every non-zero is kept. Spots with no dose get empty columns.
 *
 * rtd_field_dose_influence       computes Dij and keeps it on the device as CSC: col_ptr int64[n_spots + 1], row_idx int32[nnz]
 *                                (strictly ascending within a column), values float32[nnz]; returns nnz. No prior compute is needed.
 *                                Bitwise reproducible: the same field, inputs and threshold give the same arrays. No side effects: on
 *                                return, the field's BEV dose, its state record and everything a later rtd_field_transfer*,
 *                                rtd_field_clear_dose* or rtd_field_spot_gradient reads are those of a compute at the field's own
 *                                weights (the call ends with one). Synchronous. The CSC lives with the field: the next call replaces it,
 *                                release or destroy frees it. RTD_ERR_INVALID_ARG for nuclear_corr, a remote field, a null pointer or a
 *                                threshold outside [0, 1); RTD_ERR_RADIUS_OVERFLOW as rtd_field_finish. Not on the rtd_plan_* path.
 * rtd_field_dose_influence_copy  copies the last result; the three pointers may be host or device memory.
 * rtd_field_set_spot_weights     new spot weights [L][ny][nx] (device memory), copied on the handle's stream. What the field learned
 *                                from its last compute about its weights (uniform-sigma and radius hints) is forgotten, its trace
 *                                and plan, which do not depend on them, are kept; the next rtd_field_compute gives, bit for bit, what a fresh
 *                                rtd_field_create with these weights gives. Not for remote fields.
 * rtd_field_fetch name of the last Dij call: "dij_batch" [L][ny][nx] int32, the batch each spot was computed in (-1: empty column).
 */
int rtd_field_dose_influence(rtd_handle h, rtd_field f, float rel_threshold, size_t* nnz);
int rtd_field_dose_influence_copy(rtd_handle h, rtd_field f, int64_t* col_ptr, int32_t* row_idx, float* values);
int rtd_field_set_spot_weights(rtd_handle h, rtd_field f, const float* dev_spot_weights);

/*
 * ---- Products with the resident Dij: Dij w and Dij^T g on the device ----
 *
 * All four calls act on the matrix of the field's LAST rtd_field_dose_influence call, at the threshold it was made with, where it
 * lies (no copy to the host): RTD_ERR_NOT_READY before any such call; RTD_ERR_INVALID_ARG for a null pointer or a remote field. The
 * matrix does not depend on the spot weights: rtd_field_set_spot_weights leaves it, and what prepare built, valid. A new
 * rtd_field_dose_influence call replaces both. Device pointers are memory of this handle's device; w and the result of apply_t are
 * float32 [L][ny][nx] as spot_weights, g and the dose volume float32 on the field's dose grid. Not on the rtd_plan_* path.
 *
 * rtd_field_dose_influence_prepare  builds, once per matrix, what the products need: a row-major companion of the matrix over the
 *                                   voxels of the field's dose box (the box rtd_field_clear_dose clears; grown to the bounding box of
 *                                   the matrix's rows should spots of weight 0 reach beyond it), every row's entries in ascending column
 *                                   order, and the chunk tables of the columns. Allocates, and keeps until the matrix is replaced or
 *                                   the field released or destroyed: 8 bytes per entry (int32 column + float32 value: the matrix's
 *                                   footprint once more), 8 bytes per box voxel + 8 (int64 row pointers), 4 bytes per spot + 4, and 8
 *                                   bytes per column chunk of 2048 entries; 4 bytes per box voxel more while it runs. Synchronous and
 *                                   deterministic. A second call is a no-op.
 * rtd_field_dose_influence_apply    s[v] = sum_j Dij[v][j] * w[j]. init == 0: dev_dose[v] += s[v] for the voxels that have entries,
 *                                   no other voxel is touched (the counterpart of rtd_field_transfer: the fields of a plan are applied
 *                                   one after the other into one volume). init != 0: every voxel of the box above is WRITTEN with s[v]
 *                                   or 0 and nothing outside it is touched (the counterpart of rtd_field_transfer_init).
 * rtd_field_dose_influence_apply_t  WRITES dev_spot_grad[j] = sum_v Dij[v][j] * g[v], as rtd_field_spot_gradient does; empty columns
 *                                   give +0.
 * rtd_field_dose_influence_device   the device pointers of the CSC arrays (col_ptr int64[n_spots + 1], row_idx int32[nnz], values
 *                                   float32[nnz]) and nnz, for callers with a GPU solver of their own. No copy: the arrays are owned by
 *                                   the field and valid until its next rtd_field_dose_influence, release or destroy.
 *
 * Determinism: every output element is a float32 sum of separately rounded float32 products, in an order fixed by the matrix alone.
 * apply: the entries of row v in ascending column order are dealt to 16 lanes (entry i to lane i mod 16), each lane adds its entries
 * in order, and the 16 lane sums are added in a butterfly (distances 8, 4, 2, 1). apply_t: column j is cut into chunks of 2048
 * consecutive entries; within a chunk entry i goes to lane i mod 64, each lane adds in order, the 64 lane sums are added in a butterfly
 * (32, ..., 1); the chunk sums of a column are added the same way (chunk c to lane c mod 64). No float atomics: the same inputs give
 * the same bits across calls, handles and processes.
 *
 * Stream behaviour: after prepare, apply and apply_t only launch kernels on the handle's stream (no allocation, no host
 * synchronisation, no copy), so they can be captured into a graph like rtd_field_compute. An apply or apply_t without a prior prepare
 * runs it first, and is synchronous that once. With an all-empty matrix nothing is launched where nothing is to be written.
 */
int rtd_field_dose_influence_prepare(rtd_handle h, rtd_field f);
int rtd_field_dose_influence_apply(rtd_handle h, rtd_field f, const float* dev_spot_weights, float* dev_dose, int init);
int rtd_field_dose_influence_apply_t(rtd_handle h, rtd_field f, const float* dev_voxel_weights, float* dev_spot_grad);
int rtd_field_dose_influence_device(rtd_handle h, rtd_field f, const int64_t** col_ptr, const int32_t** row_idx, const float** values,
                                    size_t* nnz);

/*
 * ---- Products with P right-hand sides: one read of the matrix for a set of plans ----
 *
 * Additive to the block above (RTD_ABI_VERSION stays 3; the four calls above are untouched). The two products move the matrix's 8
 * bytes per entry and little else; P vectors that share the matrix share that read.
 *
 * Layout: PLAN-MINOR. Element i of plan p is at x[i * plan_stride + p], for w, the dose volume, g and the spot gradient alike, with
 * 1 <= n_plans <= plan_stride <= RTD_PLANSET_MAX_PLANS. The slots p >= n_plans are padding: no output depends on them and none of
 * them is ever written. The gather behind a matrix entry (w at a column, g at a row) is then one contiguous run of 4 * plan_stride
 * bytes; with plan_stride 1, 2, 4, 8 or 16 and dev_w (apply) or dev_g (apply_t) aligned to min(16, 4 * plan_stride) bytes it is one
 * or more vector loads (the padding is then loaded, and dropped). Any other stride or alignment is served by scalar loads of the
 * n_plans slots alone.
 *
 * rtd_field_dose_influence_apply_set    for every p < n_plans the slots p of dev_dose receive, BIT FOR BIT, what
 *                                       rtd_field_dose_influence_apply gives for plan p's vector alone, init meaning per slot what it
 *                                       means there (init == 0: the voxels without entries are not touched; init != 0: every voxel of
 *                                       the row box is written, nothing outside it).
 * rtd_field_dose_influence_apply_t_set  likewise rtd_field_dose_influence_apply_t: dev_spot_grad[j * plan_stride + p] is written for
 *                                       every spot j and p < n_plans; empty columns give +0.
 * The trees are those stated above, per plan: 16 lanes per row with the butterfly 8, 4, 2, 1; 64 lanes per chunk of 2048 entries;
 * the chunk sums added the same way; every product rounded before it is added; no float atomics. The butterflies are carried out so
 * that a lane ends with ONE plan's sum (at every distance below the number of plans a lane keeps half of its sums and receives its
 * partner's contributions to them): float addition is commutative, so these are the pairs and the bits of the plain butterfly. Only
 * the payload of a NaN that meets a NaN may differ.
 * They use the companion and the chunk tables rtd_field_dose_influence_prepare builds and add nothing per matrix. After prepare they
 * only launch on the handle's stream and can be captured; without one they run it first (synchronous that once). apply_t_set keeps
 * its chunk sums [chunk][plan_stride rounded up to 1, 2, 4, 8, 16] in a block owned by the HANDLE (4 to 64 bytes per column chunk of
 * the largest call so far): a call that needs more than any call before it allocates a larger one and cannot be captured that once;
 * outgrown blocks are kept until rtd_destroy, so a graph captured earlier stays valid.
 * That block is ONE per handle, and its users are ordered by the handle's stream alone: apply_t_set calls of one handle must not run
 * on two streams at once. After rtd_set_stream, or before a graph that holds such calls is replayed on another stream than the one
 * the handle launches on, the caller orders the two streams himself (an event, or a synchronisation), as for any buffer both use.
 * A plan set does not use that block: it owns its chunk sums.
 * They refuse what the plain calls refuse (RTD_ERR_NOT_READY without a matrix; RTD_ERR_INVALID_ARG for a null pointer or a remote
 * field) and, with RTD_ERR_INVALID_ARG, n_plans == 0, n_plans > plan_stride or plan_stride > RTD_PLANSET_MAX_PLANS.
 */
#define RTD_PLANSET_MAX_PLANS 16
int rtd_field_dose_influence_apply_set(rtd_handle h, rtd_field f, const float* dev_w, float* dev_dose, uint32_t n_plans, uint32_t plan_stride,
                                       int init);
int rtd_field_dose_influence_apply_t_set(rtd_handle h, rtd_field f, const float* dev_g, float* dev_spot_grad, uint32_t n_plans,
                                         uint32_t plan_stride);

/*
 * ---- Dose objectives and the resident spot-weight optimiser ----
 *
 * rtd_objective: structures (ROIs: sets of voxels of one dose grid) and penalty terms on them; from a dose volume on the device to
 * the objective value, the value of every term and the voxel gradient g = df/dd, without leaving the device. The gradient is what
 * rtd_field_dose_influence_apply_t takes. A term's value is weight / N_roi * sum_{v in roi} phi(d[v]) with phi by kind:
 *     RTD_OBJ_SQ_DEVIATION (d - level)^2, RTD_OBJ_SQ_OVERDOSE max(d - level, 0)^2, RTD_OBJ_SQ_UNDERDOSE min(d - level, 0)^2,
 *     RTD_OBJ_MEAN d (level ignored);
 * the objective is the sum of its terms. ROIs may overlap. At most RTD_OBJ_MAX_TERMS terms.
 *
 * rtd_objective_create    an empty objective on the dose grid dose_dims.
 * rtd_objective_add_roi   voxels: host memory, n >= 1 linear voxel indices (x fastest), strictly ascending, copied; *roi_id receives
 *                         the ROI's number (0, 1, ... in the order added).
 * rtd_objective_add_term  kind, roi (a number add_roi returned), weight > 0, dose_level (finite).
 * rtd_objective_eval      dev_dose: float32 volume on the grid; dev_values: float64[1 + terms], [0] the objective, [1 + t] term t;
 *                         dev_voxel_grad: float32 volume on the grid, WRITTEN at every voxel of the union of the ROIs (0 where a
 *                         voxel's ROIs carry no term) and touched NOWHERE else: the caller zeroes that volume once. The first eval after
 *                         an add_roi / add_term builds the device tables (the union of the ROIs ascending and, per union voxel, its
 *                         terms in term order) and is synchronous that once; every other eval is two launches on the handle's stream:
 *                         no allocation, no copy, no host synchronisation; it can be captured into a graph.
 * rtd_objective_destroy   frees it (before rtd_destroy of its handle; not while an optimiser uses it).
 * RTD_ERR_INVALID_ARG: a null pointer, a zero dimension or more than 2^31 - 1 voxels, an empty ROI, indices not strictly ascending or
 * out of range, an unknown kind or ROI, a weight that is not positive and finite, a level that is not finite, a 65th term, eval of an
 * objective without terms. After a refusal the objective is what it was.
 *
 * Arithmetic of eval (fixed, so that it can be restated): d[v] is widened to float64. With x = d[v] - level (float64), clamped as the
 * kind says (x < 0 ? 0 : x for OVERDOSE, x > 0 ? 0 : x for UNDERDOSE; a NaN stays a NaN), c_t = 2.0 * weight_t / N_t and
 * wn_t = weight_t / N_t computed once on the host in float64: g[v] = float32(sum over the voxel's terms, in term order, starting from
 * 0.0, of c_t * x, or of wn_t for a MEAN term), every product and sum in float64 without contraction, rounded once. Values: one
 * thread per union voxel, blocks of 256; the phi of term t are added over each wave of 64 by a butterfly (lane distances 32, ..., 1),
 * the four wave sums of a block as (w0 + w1) + (w2 + w3); a second launch adds the block sums of a term (block b to lane b mod 64,
 * each lane in ascending order, butterfly), multiplies by wn_t, and adds the terms in term order. float64 throughout, no atomics: the
 * same inputs give the same bits across calls, handles and processes.
 *
 * rtd_optimizer: spectral projected gradient descent (Barzilai-Borwein steps, projection on w >= 0) on an objective of the dose of
 * 1 .. RTD_OPT_MAX_FIELDS local fields of one handle on one dose grid, each with a matrix from rtd_field_dose_influence
 * (RTD_ERR_NOT_READY without; create runs rtd_field_dose_influence_prepare where it has not run). Everything the iteration touches
 * lives on the device and belongs to the optimiser: one dose volume and one g volume (zeroed at creation), w, w_prev, grad, grad_prev,
 * w_best (float32, the fields' [L][ny][nx] maps concatenated in list order), a float64 history and a record of scalars. The fields,
 * their matrices and the objective must outlive it unchanged.
 *
 * One iteration k, every step a launch on the handle's stream, no decision taken on the host:
 *   1. dose = sum_f Dij_f w_f: bit for bit a zeroed volume followed by rtd_field_dose_influence_apply(init = 0) of the fields in list
 *      order (field 0 writes its box with init = 1 after the boxes of the other fields have been cleared: the same bits);
 *   2. rtd_objective_eval -> f_k, g; history[k] = f_k while k < history_capacity;
 *   3. grad_f = Dij_f^T g (rtd_field_dose_influence_apply_t) per field;
 *   4. if f_k < f_best (+inf at the start): w_best = w, f_best = f_k, best_iteration = k;
 *   5. the step length alpha (float64). Without a Barzilai-Borwein pair (the first iteration, and the one after a guard, 7.):
 *      m = max_j |P(w - grad)_j - w_j| with P the clamp at 0, evaluated in float64 without cancellation as w_j - grad_j < 0 ? |w_j| :
      |grad_j| (a gradient can be 1e-15 of a weight); alpha = m > 0 ? 1 / m : 0 (a stationary start: alpha = 0).
 *      Else s = w - w_prev, y = grad - grad_prev (float64 differences of the float32 values), alpha = <s, s> / <s, y> if <s, y> > 0,
 *      else step_max; clamped to [step_min, step_max]. The dot products in float64 by a fixed tree: chunks of 2048 entries, one wave
 *      each, lane t adds the entries t, t + 64, ... in order, butterfly (32, ..., 1); the chunk sums are added the same way;
 *   6. w_prev = w, grad_prev = grad, w = P(w - float32(alpha) * grad) in float32 (P(x) = x > 0 ? x : +0), the product rounded before the subtraction;
 *   7. guard: if f_k is not finite, 4.-6. do not happen; w = w_best, the pair is forgotten, the next iteration takes the first rule.
 *
 * rtd_optimizer_create       options may be NULL (rtd_default_optimizer_options: step_min 1e-30, step_max 1e30, history_capacity
 *                            4096). w and w_best start as each field's own spot weights. Synchronous.
 * rtd_optimizer_set_weights  dev_w: [L][ny][nx] float32 of field field_index, copied on the stream into w. Before the first run it
 *                            sets w_best too (the start weights); later it keeps w_best, f_best and the Barzilai-Borwein pair.
 * rtd_optimizer_run          launches n_iterations iterations; asynchronous, launches only (no allocation, copy or synchronisation: a
 *                            run can be captured into a graph). A later run continues where the last stopped. n_iterations = 0: no-op.
 * rtd_optimizer_result       waits for the stream; report and the first min(capacity, report.history_len) history entries to host
 *                            memory (history may be NULL with capacity 0). RTD_ERR_INVALID_ARG (report still filled) when an iterate
 *                            was not finite before any finite one had been seen: the start itself is unusable.
 * rtd_optimizer_weights      asynchronous copy of field field_index's part of w (best == 0) or w_best (best != 0) to dev_w_out.
 * rtd_optimizer_dose         the optimiser's own volume. After a run it holds the dose of the iterate that ENTERED the last iteration
 *                            (the one f_last belongs to), not of the updated w.
 * RTD_ERR_INVALID_ARG: a null pointer, 0 or more than 16 fields, a remote field, fields of different dose grids, an objective on
 * other dims or without terms, a field index out of range, step_min > step_max or not positive. After a refusal every object stays
 * usable. Not available: nuclear_corr, remote fields, the rtd_plan_* path (as the matrix itself).
 */
enum { RTD_OBJ_SQ_DEVIATION = 0, RTD_OBJ_SQ_OVERDOSE = 1, RTD_OBJ_SQ_UNDERDOSE = 2, RTD_OBJ_MEAN = 3 };
#define RTD_OBJ_MAX_TERMS 64
#define RTD_OPT_MAX_FIELDS 16

typedef struct rtd_objective_term {
    int32_t kind;          /* RTD_OBJ_* */
    int32_t roi;           /* as returned by rtd_objective_add_roi */
    double weight;         /* > 0 */
    double dose_level;     /* in the unit of the dose volume; ignored by RTD_OBJ_MEAN */
} rtd_objective_term;

typedef struct rtd_optimizer_options {
    double step_min;            /* bounds of the Barzilai-Borwein step: they only keep it finite */
    double step_max;
    uint32_t history_capacity;  /* objective values kept on the device (later iterations are not recorded) */
    int32_t reserved[3];
} rtd_optimizer_options;

typedef struct rtd_optimizer_report {
    double f_last;              /* objective of the iterate that entered the last iteration */
    double f_best;              /* smallest finite objective seen (+inf before any) */
    double step;                /* alpha of the last iteration (unchanged by a guarded one) */
    int64_t best_iteration;     /* iteration (0-based, counted over all runs) whose iterate is w_best; -1 before any */
    uint32_t iterations;        /* iterations run so far */
    uint32_t history_len;       /* min(iterations, history_capacity) */
    int32_t guarded;            /* iterations that took the guard */
    int32_t reserved[3];
} rtd_optimizer_report;

typedef struct rtd_objective_s* rtd_objective;
typedef struct rtd_optimizer_s* rtd_optimizer;

int rtd_objective_create(rtd_handle h, const uint32_t dose_dims[3], rtd_objective* out);
int rtd_objective_add_roi(rtd_handle h, rtd_objective obj, const int32_t* voxels, size_t n, int32_t* roi_id);
int rtd_objective_add_term(rtd_handle h, rtd_objective obj, const rtd_objective_term* t);
int rtd_objective_eval(rtd_handle h, rtd_objective obj, const float* dev_dose, double* dev_values, float* dev_voxel_grad);
int rtd_objective_destroy(rtd_handle h, rtd_objective obj);

void rtd_default_optimizer_options(rtd_optimizer_options* out);
int rtd_optimizer_create(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o,
                         rtd_optimizer* out);
int rtd_optimizer_set_weights(rtd_handle h, rtd_optimizer opt, uint32_t field_index, const float* dev_w);
int rtd_optimizer_run(rtd_handle h, rtd_optimizer opt, uint32_t n_iterations);
int rtd_optimizer_result(rtd_handle h, rtd_optimizer opt, rtd_optimizer_report* r, double* history, uint32_t capacity);
int rtd_optimizer_weights(rtd_handle h, rtd_optimizer opt, uint32_t field_index, float* dev_w_out, int best);
int rtd_optimizer_dose(rtd_handle h, rtd_optimizer opt, const float** dev_dose);
int rtd_optimizer_destroy(rtd_handle h, rtd_optimizer opt);

/*
 * ---- Dose-volume histograms and DVH-point objectives ----
 *
 * Additive to the block above (RTD_ABI_VERSION stays 3): what a dose volume does to a structure in dose-volume terms, evaluated and
 * penalised on the device.
 *
 * Dose at volume. For a ROI of N voxels and a volume fraction v in (0, 1], D_v is the k-th LARGEST float32 dose of the ROI with
 * k = min(N, max(1, ceil(v * N))), the product in float64, computed once on the host. The order is that of the monotone key of a
 * float (its bits, the sign bit flipped for non-negative values, all bits flipped for negative ones), compared as an unsigned number:
 * D_v is a value that occurs in the ROI, ties cannot make it ambiguous, -0 sorts below +0 and NaNs sort by their bits (a NaN with the
 * sign bit clear above +inf, one with it set below -inf). v = 1 gives the minimum of the ROI, any v <= 1 / N the maximum.
 *
 * rtd_objective_add_dvh_term     a term of kind RTD_OBJ_MAX_DVH or RTD_OBJ_MIN_DVH. It counts towards RTD_OBJ_MAX_TERMS and takes the
 *                                next term number, mixed with the terms of rtd_objective_add_term in the order added. Its value is
 *                                weight / N * sum x^2 and it adds c_t * x to g[v] at its place in the voxel's term order, with
 *                                D = double(D_v of the dose being evaluated), d = double(dose[v]), level = dose_level and
 *                                    RTD_OBJ_MAX_DVH  x = (d > level && d <= D) ? d - level : 0   ("at most a fraction v above level":
 *                                                     satisfied, value 0, when D <= level),
 *                                    RTD_OBJ_MIN_DVH  x = (d < level && d >= D) ? d - level : 0   ("at least a fraction v receives
 *                                                     level": satisfied when D >= level);
 *                                a NaN d gives x = d, so a dose that is not finite still gives an objective that is not finite and the
 *                                optimiser's guard acts as before. D is held constant in the gradient (the usual treatment of
 *                                dose-volume penalties). The sums are those of rtd_objective_eval; the four kinds above are unchanged.
 * rtd_objective_dose_at_volume   queries: host memory, 1 <= n <= RTD_DVH_MAX_QUERIES of (roi, volume_fraction; reserved = 0);
 *                                dev_out[q] = D_v of query q (float32, device). The ranks travel as kernel arguments: once the tables
 *                                exist the call is four launches on the handle's stream (no allocation, copy or synchronisation) and
 *                                can be captured into a graph.
 * rtd_objective_dvh              the cumulative histogram of every ROI: dev_counts[roi * n_bins + b] (uint32, device) = the number of
 *                                voxels of the ROI with double(d) >= edge(b), edge(b) = (b * dose_max) / n_bins evaluated in float64
 *                                (product first). Exact. 1 <= n_bins <= 4096, dose_max finite and > 0. A NaN dose is in no bin. A
 *                                clear of dev_counts and two launches on the handle's stream.
 * rtd_objective_eval             of an objective with DVH terms: the selection (four launches, shared by all its DVH terms) in front
 *                                of the two launches of before: still no allocation, copy or host synchronisation after the first
 *                                eval, still capturable, so rtd_optimizer_run keeps its guarantees. An objective without DVH terms
 *                                launches what it launched before.
 * The first of these calls after an add_roi builds the ROI index lists on the device and is synchronous that once.
 *
 * Selection: a radix select on the keys (three passes over digits of 11, 11 and 10 bits, most significant first). Each pass counts the
 * digit of the keys that carry the digits found so far, per block in LDS, merged into one histogram per selection; the digit that
 * holds rank k is found by a descending scan of the bins. All counting is integer addition, which is associative: unlike a float
 * atomic, the order in which blocks arrive cannot change the result. The same inputs give the same bits across calls, handles and
 * processes.
 *
 * RTD_ERR_INVALID_ARG: a null pointer, a kind other than the two (and either of the two passed to rtd_objective_add_term), an unknown
 * ROI, a weight that is not positive and finite, a level that is not finite, a fraction outside (0, 1], a 65th term, n = 0 or
 * n > RTD_DVH_MAX_QUERIES, n_bins or dose_max out of range. After a refusal the objective is what it was.
 */
enum { RTD_OBJ_MAX_DVH = 4, RTD_OBJ_MIN_DVH = 5 };   /* accepted by rtd_objective_add_dvh_term only */
#define RTD_DVH_MAX_QUERIES 64

typedef struct rtd_objective_dvh_term {
    int32_t kind;             /* RTD_OBJ_MAX_DVH or RTD_OBJ_MIN_DVH */
    int32_t roi;
    double weight;            /* > 0 */
    double dose_level;
    double volume_fraction;   /* in (0, 1] */
} rtd_objective_dvh_term;

typedef struct rtd_dvh_query {
    int32_t roi;
    int32_t reserved;
    double volume_fraction;   /* in (0, 1] */
} rtd_dvh_query;

int rtd_objective_add_dvh_term(rtd_handle h, rtd_objective obj, const rtd_objective_dvh_term* t);
int rtd_objective_dose_at_volume(rtd_handle h, rtd_objective obj, const float* dev_dose, const rtd_dvh_query* queries, uint32_t n,
                                 float* dev_out);
int rtd_objective_dvh(rtd_handle h, rtd_objective obj, const float* dev_dose, uint32_t n_bins, double dose_max, uint32_t* dev_counts);

/*
 * ---- Generalised equivalent uniform dose and EUD objectives ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; rtd_objective_term and rtd_objective_dvh_term keep their layouts): the gEUD
 * of a structure, reported and penalised on the device. "The parotid's gEUD with a = 1 below 26 Gy", "the cord's near-maximum
 * (a = 16) below 45 Gy", "the target's cold-spot dose (a = -10) at least 95 %".
 *
 * Arithmetic (the contract; everything is float64). For a term or query on a ROI of N voxels, with L = dose_level (the level of a
 * term, the normalisation of a query), a = exponent, lo = 2^-15 and hi = 2^15:
 *   1. x_i = double(d_i) / L; if x_i < lo then x_i = lo; if x_i > hi then x_i = hi. A NaN fails both comparisons and stays a NaN: the
 *      objective is then not finite and the optimiser's guard acts as before. Voxel i is CLAMPED when either comparison was true.
 *   2. p_i = pow(x_i, a). With |a| <= 64 it lies in [2^-960, 2^960]: sums of up to 2^31 such values do not overflow, nothing
 *      underflows, and a zero or negative dose under a negative exponent is harmless (it is clamped to lo first).
 *   3. S = (sum_i p_i) / N, summed by one fixed tree (chunks of 2048 ROI voxels: thread t of 256 adds the chunk's voxels t, t + 256,
 *      ... in order, wave butterfly (32, ..., 1), the four waves as (0 + 1) + (2 + 3); the chunk sums the same way, chunk c to thread
 *      c mod 256). E = L * pow(S, 1 / a): the generalised equivalent uniform dose. a = 1 is the mean, a -> +inf the maximum, a -> -inf
 *      the minimum of the ROI.
 *   4. y = E - L; RTD_OBJ_SQ_MAX_EUD: y = y < 0 ? 0 : y ("E at most L"); RTD_OBJ_SQ_MIN_EUD: y = y > 0 ? 0 : y ("E at least L");
 *      RTD_OBJ_SQ_EUD keeps y. values[1 + t] = weight * y * y: not divided by N, E is a mean already.
 *   5. Gradient: K = ((2 * weight * y) * E) / ((L * double(N)) * S), evaluated once per term in exactly that association. Voxel i of
 *      the ROI adds K * (p_i / x_i) to g[v] if it is not clamped; a clamped voxel adds +0.0 (the subgradient of the clamp), and every
 *      voxel adds +0.0 when y == 0. p_i is the pow of step 2 evaluated again on the same x_i and a: the same bits. The additions per
 *      voxel are in term order, from 0.0, rounded to float32 once, as for every other kind.
 * No float atomics: the same inputs give the same bits across calls, handles, processes and graph replays. The device's pow is the
 * device library's; a host restatement agrees within that function's error bound, not bit for bit.
 *
 * rtd_objective_add_eud_term   a term of kind RTD_OBJ_SQ_EUD, _SQ_MAX_EUD or _SQ_MIN_EUD. It counts towards RTD_OBJ_MAX_TERMS and takes
 *                              the next term number, mixed with the terms of the two other add_* calls in the order added.
 * rtd_objective_eud            queries: host memory, 1 <= n <= RTD_EUD_MAX_QUERIES of (roi, dose_level = L, exponent; reserved = 0);
 *                              dev_out[q] = E of query q (float64, device). The parameters travel as kernel arguments: once the
 *                              tables exist the call is two launches on the handle's stream (no allocation, copy or synchronisation)
 *                              and can be captured into a graph. The first call after an add_roi builds the ROI index lists
 *                              (shared with the dose-volume calls) and is synchronous that once.
 * rtd_objective_eval           of an objective with EUD terms: after the DVH selection (if it has DVH terms) two launches (the sums,
 *                              then E, K and the value of every EUD term) in front of the two of before; still no allocation, copy
 *                              or host synchronisation after the first eval, still capturable. An objective without EUD terms
 *                              launches what it launched before and gives the same bits.
 * rtd_optimizer_create, _create_robust: accept such objectives (a scenario is evaluated like any dose). rtd_optimizer_create_voxelwise
 * and rtd_objective_eval_voxelwise refuse them: E couples the voxels of a ROI, so the objective of the per-voxel worst dose is not
 * the sum over voxels the voxel-wise composite needs.
 *
 * RTD_ERR_INVALID_ARG: a null pointer, a kind other than the three (and any of the three passed to rtd_objective_add_term or
 * rtd_objective_add_dvh_term), an unknown ROI, a weight that is not positive and finite, a dose_level that is not finite or not
 * greater than 0, an exponent that is not finite or with |exponent| outside [2^-4, 64], reserved != 0, a 65th term, n = 0 or
 * n > RTD_EUD_MAX_QUERIES. After a refusal the objective is what it was.
 */
enum { RTD_OBJ_SQ_EUD = 6, RTD_OBJ_SQ_MAX_EUD = 7, RTD_OBJ_SQ_MIN_EUD = 8 };   /* accepted by rtd_objective_add_eud_term only */
#define RTD_EUD_MAX_QUERIES 64

typedef struct rtd_objective_eud_term {
    int32_t kind;             /* RTD_OBJ_SQ_EUD, RTD_OBJ_SQ_MAX_EUD or RTD_OBJ_SQ_MIN_EUD */
    int32_t roi;
    double weight;            /* > 0 */
    double dose_level;        /* L: finite, > 0 */
    double exponent;          /* a: 2^-4 <= |a| <= 64 */
    double reserved;          /* 0 */
} rtd_objective_eud_term;

typedef struct rtd_eud_query {
    int32_t roi;
    int32_t reserved;
    double dose_level;        /* the normalisation L: finite, > 0; any dose of the ROI's order of magnitude */
    double exponent;          /* a: 2^-4 <= |a| <= 64 */
} rtd_eud_query;

int rtd_objective_add_eud_term(rtd_handle h, rtd_objective obj, const rtd_objective_eud_term* t);
int rtd_objective_eud(rtd_handle h, rtd_objective obj, const float* dev_dose, const rtd_eud_query* queries, uint32_t n, double* dev_out);

/*
 * ---- Robust spot-weight optimisation over error scenarios ----
 *
 * Additive to the two blocks above (RTD_ABI_VERSION stays 3). A scenario is one realisation of the plan under an error: the same
 * spot maps on a displaced geometry (a set-up error) or under LUTs with a scaled stopping-power table (a range error). To the engine
 * it is just another list of fields, each with its own matrix from rtd_field_dose_influence. A robust optimiser holds S scenarios of
 * F fields and ONE weight vector (the F spot maps concatenated, shared by all scenarios), and minimises either the expected value or
 * the worst case of the objective over the scenarios.
 *
 * rtd_optimizer_create_robust   fields: n_scenarios x n_fields handles, scenario-major; scenario 0 is by convention the nominal one.
 *                               Field f of every scenario must have the spot-map shape (nx, ny, L) of field f of scenario 0. Start
 *                               weights are those of scenario 0's fields. Returns an ordinary rtd_optimizer: rtd_optimizer_set_weights,
 *                               _run, _result, _weights, _dose (scenario 0) and _destroy work on it unchanged. On top of what a plain
 *                               optimiser owns it allocates a dose and a g volume per further scenario (2 S volumes in all), S
 *                               per-scenario spot gradients and the record below. Synchronous. The environment variable
 *                               RTD_ROBUST_NO_BATCH, read once here, makes the optimiser issue the single-matrix launches of the plain
 *                               iteration scenario by scenario instead of the launches batched over the scenario axis: the same bits.
 * rtd_optimizer_scenario_values waits for the stream; f_s, lambda_s (may be NULL) and the worst scenario s* (may be NULL; under
 *                               EXPECTED the lowest index holding the maximum as well) of the iterate f_last belongs to; zeros before
 *                               the first run. On a plain optimiser: one scenario, values[0] = f_last, lambda 1.0, worst 0.
 * rtd_optimizer_scenario_dose   scenario s's own volume: after a run the dose of the iterate that entered the last iteration under
 *                               scenario s. On a plain optimiser scenario 0 is rtd_optimizer_dose.
 *
 * One iteration k, every step a launch on the handle's stream, no decision taken on the host:
 *   1. for every scenario s: dose_s = sum_f Dij_{s,f} w_f, into the scenario's own volume: bit for bit a zeroed volume followed by
 *      rtd_field_dose_influence_apply(init = 0) of that scenario's fields in list order (step 1 above, per scenario);
 *   2. for every scenario s: rtd_objective_eval(dose_s) -> f_s, its term values, g_s (own volume, zeroed once at creation). The
 *      objective's scratch (DVH thresholds, partial sums) is shared: the evals run one after the other on the stream;
 *   3. one launch decides. EXPECTED: lambda_s = p_s, F = sum_s p_s * f_s in float64, ascending s, starting from 0.0, every product
 *      rounded before it is added. WORST_CASE: s* is the lowest index with f_s == max_s f_s, lambda_{s*} = 1.0, the others 0.0,
 *      F = f_{s*}. If any f_s is not finite, s* is the lowest such index and F = f_{s*} in either mode (the guard, 7., then acts).
 *      lambda, f_s and s* are kept in the optimiser's device record; history[k] = F_k while k < history_capacity;
 *   4. for every scenario with lambda_s != 0: grad_s = Dij_{s,f}^T g_s per field, float32, as rtd_field_dose_influence_apply_t writes it;
 *   5. grad[j] = float32(sum over the scenarios with lambda_s != 0, ascending s, of lambda_s * double(grad_s[j])): a float64 sum of
 *      separately rounded products that STARTS FROM THE FIRST PRODUCT, not from 0.0, rounded once. With one scenario and lambda 1.0
 *      the result is grad_0[j] to the bit, a -0 included;
 *   6. steps 4.-7. of the iteration above, word for word, with f_k := F_k and grad := the combined gradient.
 * With n_scenarios = 1, EXPECTED and p = 1.0 this is the plain iteration bit for bit.
 *
 * Launches: per field position one launch covers that position in all scenarios (the grid has a scenario dimension, the per-scenario
 * operands travel as one kernel argument); the blocks of a scenario whose lambda_s, read from the device record, is 0 leave the
 * transposed product at once, so under WORST_CASE only the worst scenario's transposed product does work. Per output element the
 * lane assignment, the order of the additions and the butterflies are those of the single-matrix products. As rtd_optimizer_run of a
 * plain optimiser: launches only, no allocation, copy or host synchronisation, capturable into a graph, no float atomics, every
 * order of summation fixed by the inputs alone: the same bits across calls, handles and processes.
 *
 * RTD_ERR_INVALID_ARG: a null pointer, an unknown mode, 0 or more than RTD_ROBUST_MAX_SCENARIOS scenarios, 0 or more than 16 fields
 * per scenario, a probability that is not positive and finite, a remote field, a field listed twice (a field's product workspace is
 * its own, and the batched launches would share it), a spot-map shape that differs between scenarios, fields of different dose grids,
 * an objective on other dims or without terms, a scenario index out of range. RTD_ERR_NOT_READY: a field without a matrix. After a
 * refusal every object stays usable. Not available: nuclear_corr, remote fields, the rtd_plan_* path (as the matrix itself).
 */
enum { RTD_ROBUST_EXPECTED = 0, RTD_ROBUST_WORST_CASE = 1 };
#define RTD_ROBUST_MAX_SCENARIOS 32

typedef struct rtd_robust_options {
    int32_t  mode;                /* RTD_ROBUST_*                                   */
    uint32_t n_scenarios;         /* 1 .. RTD_ROBUST_MAX_SCENARIOS                  */
    const double* probabilities;  /* [n_scenarios], each finite and > 0, used as given (not normalised);
                                     NULL: 1.0 / n_scenarios each. Ignored by WORST_CASE. Copied. */
    int32_t  reserved[4];
} rtd_robust_options;

int rtd_optimizer_create_robust(rtd_handle h, const rtd_field* fields /* [n_scenarios][n_fields], scenario-major */,
                                uint32_t n_fields, const rtd_robust_options* robust, rtd_objective obj,
                                const rtd_optimizer_options* o, rtd_optimizer* out);
int rtd_optimizer_scenario_values(rtd_handle h, rtd_optimizer opt, double* values /* host [n_scenarios] */,
                                  double* lambdas /* host [n_scenarios] or NULL */, int32_t* worst /* or NULL */);
int rtd_optimizer_scenario_dose(rtd_handle h, rtd_optimizer opt, uint32_t scenario, const float** dev_dose);

/*
 * ---- The voxel-wise worst case over error scenarios ----
 *
 * Additive to the three blocks above (RTD_ABI_VERSION stays 3; rtd_robust_options and rtd_optimizer_create_robust are untouched). The
 * block above decides per SCENARIO. Here every voxel takes, across the scenarios, the dose that is worst for each term (the composite
 * worst-case dose): over-dose penalties see the voxel's maximum, under-dose penalties its minimum, and the gradient of a voxel's
 * penalty flows back through the scenario that supplied that extreme.
 *
 * Extremes of a voxel v over the doses d_s = dose_s[v], s = 0 .. S - 1, compared as float32: hi is the largest d_s and s_hi the lowest
 * index that holds it, lo the smallest d_s and s_lo the lowest index that holds it (-0 == +0, so the lower index wins). If any d_s is a
 * NaN, hi = lo = the NaN of the lowest such s and s_hi = s_lo = that s: a dose that is not finite still gives an objective that is not
 * finite, and the optimiser's guard acts as before.
 *
 * rtd_objective_eval_voxelwise   the sibling of rtd_objective_eval on S volumes. dev_doses, dev_voxel_grads: HOST arrays of
 *                                n_scenarios device pointers (float32 volumes on the grid; read during the call only, they travel
 *                                as one kernel argument); dev_values: float64[1 + terms] as rtd_objective_eval; dev_active: one
 *                                word on the device, bit s set iff scenario s received a gradient that is not zero. Per union
 *                                voxel v and per term t of the voxel, in term order, the term sees the dose d of
 *                                    RTD_OBJ_SQ_OVERDOSE, RTD_OBJ_MEAN   (hi, s_hi),
 *                                    RTD_OBJ_SQ_UNDERDOSE                (lo, s_lo),
 *                                    RTD_OBJ_SQ_DEVIATION                (hi, s_hi) when |hi - level| >= |lo - level| in float64,
 *                                                                        else (lo, s_lo),
 *                                and phi and the contribution c_t x (wn_t for MEAN) are those of rtd_objective_eval on that d.
 *                                Gradient: the contributions at v are summed in float64, in term order, starting from 0.0, one sum
 *                                per receiving scenario; when s_hi == s_lo every term adds to ONE sum (so that with one scenario the
 *                                result is rtd_objective_eval to the bit). g_{s_hi}[v] and g_{s_lo}[v] get their sum rounded once to
 *                                float32, every other scenario's g_s[v] gets +0.0f: all S volumes are WRITTEN at every voxel of the
 *                                union of the ROIs, because the choice moves between calls, and touched nowhere else. Active word:
 *                                bit s is set iff some value written to g_s compares != 0 (a NaN does); the call clears the word
 *                                first, a wave sets its bits with one integer OR (order-free, as the DVH counts). Values: the sums
 *                                of phi per term by the tree of rtd_objective_eval, unchanged. After the objective's tables exist
 *                                the call is a clear of the word and two launches on the handle's stream: no allocation, no copy, no
 *                                host synchronisation; it can be captured into a graph. The dose at volume of a composite needs the
 *                                composite materialised first, so an objective with DVH terms is refused here (left for later);
 *                                rtd_scenario_dose_extremes materialises it for reporting.
 * rtd_scenario_dose_extremes     dev_min[v] = lo, dev_max[v] = hi (the rules above) for v < n_voxels; either output may be NULL.
 *                                One launch on the handle's stream, capturable. What rtd_objective_dvh and
 *                                rtd_objective_dose_at_volume are pointed at for worst-case DVH bands and a worst-case D95.
 * rtd_optimizer_create_voxelwise ownership, checks and refusals of rtd_optimizer_create_robust (the field list, RTD_ERR_NOT_READY
 *                                without a matrix, the same spot-map shapes and dose grid across scenarios, RTD_ROBUST_NO_BATCH);
 *                                in addition an objective with DVH terms is refused. Returns an ordinary rtd_optimizer; it owns
 *                                what a robust optimiser owns and the active word.
 *
 * One iteration k, every step a launch on the handle's stream, no decision taken on the host:
 *   1. step 1 of the block above: dose_s = sum_f Dij_{s,f} w_f into the S volumes;
 *   2. rtd_objective_eval_voxelwise on the S volumes -> F, the term values, g_s, the active word;
 *   3. one thread of one launch: lambda_s = 1.0 where bit s is set and 0.0 elsewhere; f_s = F for every s (a composite has no
 *      per-scenario split); s* = the lowest active s, or 0 if none is; history[k] = F while k < history_capacity;
 *   4. step 4 of the block above: grad_s = Dij_{s,f}^T g_s for the scenarios with lambda_s != 0;
 *   5. step 5 of the block above: grad[j] = float32(sum over the active scenarios, ascending s, of double(grad_s[j])), from the first
 *      product, rounded once; +0 when no scenario is active;
 *   6. steps 4.-7. of the plain iteration, word for word, with f_k := F_k and grad := the combined gradient.
 * With n_scenarios = 1 this is the plain iteration bit for bit. rtd_optimizer_scenario_values returns the record of step 3;
 * rtd_optimizer_scenario_dose, _dose, _weights, _result, _set_weights, _run and _destroy work as on a robust optimiser.
 *
 * RTD_ERR_INVALID_ARG: a null pointer (any entry of either array included), n_scenarios of 0 or above RTD_ROBUST_MAX_SCENARIOS, an
 * objective without terms or with DVH terms, n_voxels == 0, both outputs NULL, and whatever rtd_optimizer_create_robust refuses.
 * After a refusal every object is what it was.
 */
int rtd_objective_eval_voxelwise(rtd_handle h, rtd_objective obj,
        const float* const* dev_doses  /* host array of n_scenarios device pointers */,
        uint32_t n_scenarios           /* 1 .. RTD_ROBUST_MAX_SCENARIOS */,
        double* dev_values             /* [1 + terms], as rtd_objective_eval */,
        float* const* dev_voxel_grads  /* host array of n_scenarios device pointers */,
        uint32_t* dev_active           /* one word: bit s set iff scenario s received a non-zero gradient */);
int rtd_scenario_dose_extremes(rtd_handle h, const float* const* dev_doses, uint32_t n_scenarios,
                               size_t n_voxels, float* dev_min /* or NULL */, float* dev_max /* or NULL */);
int rtd_optimizer_create_voxelwise(rtd_handle h, const rtd_field* fields /* [n_scenarios][n_fields], scenario-major */,
                                   uint32_t n_fields, uint32_t n_scenarios, rtd_objective obj,
                                   const rtd_optimizer_options* o, rtd_optimizer* out);

/*
 * ---- RT Structure Set contours -> ROI voxel lists ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). Everything above begins at rtd_objective_add_roi, which takes strictly
 * ascending linear voxel indices of the dose grid; this block makes such a list from the closed planar contours of a structure
 * (rtd_dicom::readStructureSet and rtd_dicom::flatten of include/rtd_dicom.hpp deliver them). The mask is decided by comparisons of
 * float64 values and by integer counting only: the same inputs give the same bits across calls, handles and processes, and the rule can
 * be restated in a few lines (tests/roi_reference.py does).
 *
 * Inputs. rtd_roi_grid: the dims of the dose grid, the affine that takes a point in mm to (fractional) voxel indices (i, j, k) of
 * that grid (voxel centres at the integers), and the thickness in mm of the slab a contour plane stands for (the spacing of the
 * contoured image's slices). rtd_contour_set: n_contours closed polygons; contour c owns the points offsets[c] .. offsets[c + 1] - 1 of
 * `points` (xyz in mm, host memory); the last point closes to the first.
 *
 * Transform (host, float64, the float32 inputs widened, every product and sum rounded, nothing contracted), for a point (x, y, z):
 *     u  = ((m[0] x + m[1] y) + m[2] z) + v[0]        v = ((m[3] x + m[4] y) + m[5] z) + v[1]        kc = ((m[6] x + m[7] y) + m[8] z) + v[2]
 * Planarity: a contour's plane coordinate is the kc of its first point; the call is refused if any of its points differs from that
 *     by more than 1e-3 (slices).
 * Planes: the contours sorted stably by plane coordinate; a new plane starts when a contour's coordinate exceeds the coordinate of the
 *     plane's FIRST contour by more than 1e-3. kc_p is the coordinate of plane p's first contour.
 * Slice assignment: slab = double(plane_thickness_mm) * sqrt((m[6] m[6] + m[7] m[7]) + m[8] m[8]) (slices). Slice k takes the plane p
 *     that minimises |k - kc_p|, a tie going to the lower kc_p, and only if |k - kc_p| <= slab / 2; otherwise the slice takes no plane.
 * Inside test: even-odd over ALL edges a -> b of ALL contours of the slice's plane (nested contours are holes, overlapping contours
 *     XOR: the RTSTRUCT convention). For row j and edge a -> b in (u, v):
 *         no crossing when (av <= j) == (bv <= j); otherwise t = (j - av) / (bv - av), xc = au + t * (bu - au),
 *     every operation rounded to float64, nothing contracted; voxel i of the row is flipped iff double(i) < xc. Voxel (i, j, k) is in the
 *     ROI iff it was flipped an odd number of times. No other number enters: a vertex on a row, a horizontal edge on a row and a
 *     crossing exactly on a voxel centre are decided by these comparisons alone.
 *
 * rtd_roi_rasterize   synchronous set-up call (allocations, copies and a wait). The result owns its device memory, like an objective:
 *                     the packed mask of the covered slices and the voxel list. A structure that covers no voxel is a valid result
 *                     (n_voxels == 0); rtd_objective_add_roi goes on refusing an empty list.
 * rtd_roi_get_info    n_voxels; the inclusive bounding box of the voxels in (i, j, k) (all zero when n_voxels == 0); the number of
 *                     planes; the number of slices that took a plane.
 * rtd_roi_voxels      the list in host memory: linear indices (k ny + j) nx + i, strictly ascending. capacity (in entries) must be at
 *                     least n_voxels. Synchronous.
 * rtd_roi_device      the list on the device (owned by the ROI, valid until rtd_roi_destroy) and its length.
 * rtd_roi_fill_mask   dev_mask: dims[0] dims[1] dims[2] bytes on the device, x fastest; EVERY byte is written, 1 inside and 0 outside.
 *                     One launch on the handle's stream.
 * rtd_roi_kernel_ms   the time of the kernels of rtd_roi_rasterize that made this ROI (hipEvents on the handle's stream), for reports.
 *
 * Kernels (rtd_roi.hpp): per covered slice and group of rows the crossings toggle bits of a per-row difference mask in LDS (integer
 * atomicXor, order-free); a suffix XOR over the bits gives the row mask, stored packed; a popcount per row, an exclusive integer scan over
 * the rows in (k, j) order and an emit of the set bits give the list ascending without a sort. Slices without a plane launch nothing.
 * The only atomics are integer XOR / min / max; there are no float atomics.
 *
 * RTD_ERR_INVALID_ARG, after which every object stays usable: a null pointer, a zero dimension or more than 2^31 - 1 voxels,
 * n_contours == 0, a contour with fewer than 3 points, offsets that are not ascending, more than 2^31 - 1 points, a coordinate or
 * matrix entry that is not finite, plane_thickness_mm not positive and finite, a contour that is not planar in the grid's k, a capacity
 * below n_voxels.
 */
typedef struct rtd_roi_grid {
    uint32_t dims[3];
    rtd_affine world_to_idx;      /* mm -> voxel index (i, j, k) of the dose grid */
    float plane_thickness_mm;     /* > 0 */
    int32_t reserved[3];
} rtd_roi_grid;

typedef struct rtd_contour_set {
    const float* points;          /* host, xyz mm */
    const uint32_t* offsets;      /* host, n_contours + 1, ascending */
    uint32_t n_contours;
    int32_t reserved[3];
} rtd_contour_set;

typedef struct rtd_roi_info {
    uint64_t n_voxels;
    uint32_t box_lo[3], box_hi[3];   /* inclusive, (i, j, k) */
    uint32_t n_planes, n_slices_covered;   /* of the contour input; both 0 for a derived ROI (rtd_roi_margin, _combine, _from_mask) */
    int32_t reserved[2];
} rtd_roi_info;

typedef struct rtd_roi_s* rtd_roi;

int rtd_roi_rasterize(rtd_handle h, const rtd_roi_grid* grid, const rtd_contour_set* contours, rtd_roi* out);
int rtd_roi_get_info(rtd_handle h, rtd_roi roi, rtd_roi_info* info);
int rtd_roi_voxels(rtd_handle h, rtd_roi roi, int32_t* host_out, size_t capacity);
int rtd_roi_device(rtd_handle h, rtd_roi roi, const int32_t** dev_voxels, size_t* n);
int rtd_roi_fill_mask(rtd_handle h, rtd_roi roi, uint8_t* dev_mask);
int rtd_roi_kernel_ms(rtd_handle h, rtd_roi roi, float* ms);
int rtd_roi_destroy(rtd_handle h, rtd_roi roi);

/*
 * ---- Spots from a target: the target in beam's-eye view ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). A target on the dose grid (a byte mask, as rtd_roi_fill_mask writes it) is
 * projected into the (ray, step) grid of a computed field, and the spots whose Bragg peak lands in it are marked: the way from a
 * structure to the spot map of a field. Every decision below is a comparison of float32 values computed in the stated order, each
 * product, quotient, sum and difference rounded, nothing contracted; all counting is integer. The same inputs give the same bits across
 * calls, handles and processes, and the rule can be restated in a few lines (tests/target_reference.py does).
 *
 * Notation: W, H, L = rtd_field_info.ray_dims, S = tracer_steps, wepl[k][j][i] the field's cumulative water-equivalent depth
 * (rtd_field_fetch "wepl": a sum of non-negative terms, so it does not decrease along a ray), (nx, ny, nz) = dose_dims.
 *
 * (a) Projection. For ray (i, j), 0 <= i < W, 0 <= j < H, and step 0 <= k < S, with f = (float(i), float(j), float(k)):
 *         g = f * ray_res + ray_offset                                  (component-wise)
 *         g.x = g.x * (1.0f - g.z / source_dist[0])     g.y = g.y * (1.0f - g.z / source_dist[1])      (g.z / inf = 0)
 *         p.c = ((m[3c] * g.x + m[3c + 1] * g.y) + m[3c + 2] * g.z) + v[c]        with (m, v) = gantry_to_dose_idx, c = 0, 1, 2
 *     (Float3FromFanTransform::transformPoint, float3_from_fan_transform.cu:37-42, with the ray grid as the fan index). Nearest voxel:
 *     q.c = floorf(p.c + 0.5f). The sample is inside iff 0.0f <= q.x < float(nx), 0.0f <= q.y < float(ny), 0.0f <= q.z < float(nz)
 *     (compared as floats before any conversion; a NaN is outside) and the mask byte at ((int q.z * ny) + int q.y) * nx + int q.x is
 *     non-zero. Stored packed, uint32 [ceil(S / 32)][H][W]: bit k & 31 of word [k >> 5][j][i]; the bits of steps >= S are 0.
 * (b) Summary over all inside samples: their number; the smallest and the largest wepl[k][j][i] (0, 0 when there is none); the
 *     inclusive box of the rays (i, j) and the inclusive range of the steps k that have one (all 0 when there is none).
 * (c) Layer hit, per layer l and ray (i, j). R = the layer's peak depth (rtd_field_fetch "layer_plan", column 2),
 *     lo = R - distal_margin_mm, hi = R + proximal_margin_mm. kLo = the number of steps k with wepl[k][j][i] < lo,
 *     kHi = min(the number of steps k with wepl[k][j][i] < hi, S - 1). No hit when kLo == S (the ray never reaches that depth); otherwise
 *     a hit iff a bit of (a) is set for some step of [kLo, kHi] (lo <= hi, so the range is not empty). With both margins 0 that is the one
 *     step at which the cumulative depth first reaches the peak depth. The test is on samples, not on a proximal / distal interval: a
 *     hollow or two-part target is handled. So a layer is also taken when its peak lies up to distal_margin_mm beyond a target sample of
 *     the ray, or up to proximal_margin_mm in front of one (give or take the step in which the depth is reached).
 * (d) Spot (sx, sy) has the ray coordinates of the spot -> ray convolution:
 *         cx = (spot_offset[0] - ray_offset[0]) / ray_res[0] + float(sx) * (spot_delta[0] / ray_res[0])        cy likewise with [1], sy
 *     (spot_* = spot_idx_to_gantry; the product is rounded, then added). Its rays are the nearest ray (floorf(cx + 0.5f),
 *     floorf(cy + 0.5f)) and, when lateral_margin_mm = m > 0, every ray (i, j) with dx * dx + dy * dy <= m * m, where
 *     dx = (float(i) - cx) * ray_res[0], dy = (float(j) - cy) * ray_res[1] (the sum of the two rounded squares), both clipped to the
 *     ray grid (the nearest ray compared as floats, like (a)). Spot (l, sy, sx) is selected iff some ray of its set has a hit for l.
 *     The lateral margin is a distance in the isocentre plane, the plane of the ray grid: it ignores the divergence of the beam.
 *
 * rtd_field_project_target  dev_mask: nx ny nz bytes on this handle's device, x fastest, non-zero = inside. Stores (a) with the field,
 *                           fills info with (b); synchronous (it returns a record). The field owns the projection: a later call
 *                           replaces it, rtd_field_release and rtd_field_destroy free it. The buffers (4 bytes per ray and 32 steps,
 *                           1 byte per ray and layer) are allocated by the first call.
 * rtd_field_select_spots    (c) and (d) from the stored projection: WRITES every byte of dev_spot_mask ([L][ny][nx] as spot_weights,
 *                           device memory), 1 selected, 0 not. opt == NULL: all margins 0. Two launches on the handle's stream: no
 *                           allocation, no copy, no host synchronisation when n_selected is NULL (it can be captured into a graph);
 *                           with n_selected a third launch counts, and the call waits and returns the number of selected spots. One
 *                           projection serves any number of selections.
 * Both read the trace (wepl) and the layer records the field holds when they run — those of its last compute — and write nothing that a
 * later transfer, gradient or rtd_field_dose_influence reads. wepl_min / wepl_max bracket the peak depths worth offering to the field.
 * rtd_field_fetch names: "target_bev" uint32 [ceil(S / 32)][H][W] after a projection, "target_hit" uint8 [L][H][W], the hits (c) of
 * the last selection.
 *
 * RTD_ERR_NOT_READY: before any compute of the field; rtd_field_select_spots also before any projection. RTD_ERR_INVALID_ARG: a null
 * pointer other than opt and n_selected, a remote field, nuclear_corr, a margin that is negative or not finite. After a refusal
 * every object stays usable. Not on the rtd_plan_* path.
 */
typedef struct rtd_target_info {
    uint64_t n_samples;            /* (ray, step) samples inside the target */
    float wepl_min, wepl_max;      /* min / max of wepl over those samples (0, 0 when none) */
    int32_t ray_lo[2], ray_hi[2];  /* inclusive box of rays (i, j) with at least one sample (all 0 when none) */
    int32_t step_lo, step_hi;      /* inclusive range of steps with at least one sample */
    int32_t reserved[4];
} rtd_target_info;

typedef struct rtd_target_options {
    float lateral_margin_mm;       /* >= 0, in the isocentre plane (the ray grid's plane) */
    float proximal_margin_mm;      /* >= 0, water-equivalent mm */
    float distal_margin_mm;        /* >= 0, water-equivalent mm */
    int32_t reserved[5];
} rtd_target_options;

int rtd_field_project_target(rtd_handle h, rtd_field f, const uint8_t* dev_mask, rtd_target_info* info);
int rtd_field_select_spots(rtd_handle h, rtd_field f, const rtd_target_options* opt, uint8_t* dev_spot_mask, uint32_t* n_selected);

/*
 * ---- Gamma index of two dose volumes ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). The comparison of an evaluated dose with a reference dose on one grid: per
 * reference voxel the smallest combined distance / dose-difference measure over a search cube, with the evaluated dose interpolated
 * between grid nodes when asked. Both volumes, the optional mask and map and the result record live on the handle's device; volumes are
 * x fastest, dims and spacing_mm are (x, y, z). Every number below is a float32 operation in the stated order, each product, quotient,
 * sum and difference rounded, nothing contracted; `/` and sqrtf are correctly rounded, the minimum and the maximum are order-free and
 * all counting is integer: the same inputs give the same bits across calls, handles and processes, and the rule can be restated in a
 * few lines (tests/gamma_reference.py does).
 *
 * Normalisation. norm = norm_dose if that is > 0, otherwise the largest ref[v] over the WHOLE grid (not only the mask), starting from
 *     0.0f. thr = threshold_fraction * norm, dd_global = dd_fraction * norm. If !(norm > 0): n_evaluated = n_passed = 0, max_gamma = 0
 *     and every voxel of the map is -1.0f.
 * Radii. r_a = (int)ceilf(search_mult * dta_mm / spacing_mm[a]) per axis a, at most RTD_GAMMA_MAX_RADIUS. With k = interp the offsets
 *     are the integers i_a in [-k r_a, k r_a], in units of spacing_mm[a] / (float)k.
 * Evaluated voxels. v is evaluated iff ref[v] >= thr, and dev_mask is NULL or dev_mask[v] != 0 (a byte mask as rtd_roi_fill_mask
 *     writes it: a pass rate per structure is one call), and ref[v] > 0 when local is set.
 * Sample of voxel v = (v_x, v_y, v_z) at offset (i_x, i_y, i_z). Per axis: b = floor_div(i, k), t = (float)(i - b k) / (float)k (exact:
 *     k is a power of two), p = v_a + b. The sample is skipped if p < 0 or p > n_a - 1, or if p == n_a - 1 and t != 0. The upper
 *     neighbour is node min(p + 1, n_a - 1). e = the trilinear blend of the 8 nodes of eval, each blend a + t * (b - a) (one difference,
 *     one product, one sum), along x, then along y, then along z; with k = 1 every t is 0 and e is the node's value.
 *         o_a   = (float)i_a * (spacing_mm[a] / (float)k)
 *         dist2 = (o_x * o_x + o_y * o_y) + o_z * o_z
 *         dv    = e - r,  r = ref[v]            dd = dd_global, or dd_fraction * r when local is set
 *         g2    = dist2 / (dta_mm * dta_mm) + (dv * dv) / (dd * dd)
 * Gamma. best = the smallest g2 over the samples that are not skipped (the one at offset 0 never is), gamma = sqrtf(best); the voxel
 *     passes iff gamma <= 1.0f. max_gamma = the largest gamma (0 when nothing is evaluated).
 * With k = 1, search_mult = 1.5, no mask, global and norm_dose = 0 this is the plain node-by-node search of the test suite's CPU
 * checker, operation for operation. Inputs are finite doses; what non-finite input yields is unspecified, but nothing faults.
 *
 * rtd_default_gamma_options   1 % / 1 mm above 10 %, search_mult 1.5, global, norm_dose 0, interp 1.
 * rtd_dose_gamma              asynchronous on the handle's stream: clears *dev_result, then launches only — no allocation after the
 *                             first call, no copy, no host synchronisation (it can be captured into a graph, like the DVH calls; a
 *                             captured call is not timed). dev_gamma_map (or NULL): dims[0] dims[1] dims[2] floats, EVERY one written:
 *                             gamma where evaluated, -1.0f elsewhere. *dev_result: the counts, max_gamma and the norm that was used;
 *                             the pass rate is n_passed / n_evaluated.
 * rtd_dose_gamma_kernel_ms    the time of the search kernel of the handle's last rtd_dose_gamma (hipEvents on the handle's stream; it
 *                             waits for that kernel), for reports. RTD_ERR_NOT_READY before any call.
 *
 * Kernels (rtd_gamma.hpp): the grid maximum by an integer atomicMax on the float's bit pattern (doses are not negative); the search by
 * bricks of 32 x 4 x 4 reference voxels, one per lane, over a tile of eval with its halo staged in LDS once, the offsets visited in
 * growing distance per axis and left, per wave, once the distance term alone rules out an improvement for every lane (this cannot change
 * a minimum). Counts: ballots and popcounts kept in registers while a block walks its bricks, then per block one 64-bit integer atomicAdd per
 * counter and an integer atomicMax on the bit pattern of its largest gamma. No float atomics. Environment: RTD_GAMMA_NAIVE (read by rtd_create) selects the plain second implementation — one lane per voxel, the
 * nested loops above over global memory, no pruning — which gives the same bits.
 *
 * RTD_ERR_INVALID_ARG, after which nothing has been written: a null h, dev_ref, dev_eval, dims, spacing_mm, opt or dev_result; a zero
 * dim; a spacing, dd_fraction, dta_mm or search_mult that is not > 0 (and finite); threshold_fraction < 0; norm_dose < 0; interp not in
 * {1, 2, 4, 8}; local > 1; a non-zero reserved word; a radius above RTD_GAMMA_MAX_RADIUS.
 */
#define RTD_GAMMA_MAX_RADIUS 10u   /* search radius in grid nodes, per axis */
typedef struct rtd_gamma_options {
    float    dd_fraction;         /* 0.01 */
    float    dta_mm;              /* 1.0 */
    float    threshold_fraction;  /* 0.10 */
    float    search_mult;         /* 1.5: the search cube reaches search_mult * dta */
    float    norm_dose;           /* 0: max(ref) found on the device; > 0: this dose normalises dd and the threshold */
    uint32_t local;               /* 0 global: dd = dd_fraction * norm; 1 local: dd = dd_fraction * ref[v] */
    uint32_t interp;              /* 1, 2, 4 or 8 samples per grid step of the evaluated dose */
    uint32_t reserved[5];         /* zero */
} rtd_gamma_options;              /* 48 bytes */
typedef struct rtd_gamma_result { /* lives on the DEVICE */
    uint64_t n_evaluated, n_passed;
    float    max_gamma, norm_dose;
    uint32_t reserved[2];
} rtd_gamma_result;               /* 32 bytes */
void rtd_default_gamma_options(rtd_gamma_options* out);
int rtd_dose_gamma(rtd_handle h, const float* dev_ref, const float* dev_eval, const uint32_t dims[3], const float spacing_mm[3],
                   const rtd_gamma_options* opt, const uint8_t* dev_mask /* or NULL */, float* dev_gamma_map /* or NULL */,
                   rtd_gamma_result* dev_result);
int rtd_dose_gamma_kernel_ms(rtd_handle h, float* ms);   /* the search kernel of the last call, as rtd_roi_kernel_ms */

/*
 * ---- Derived ROIs: margins, boolean algebra, an ROI from a mask ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). The structures nobody draws: a target plus a margin, a ring around it, an
 * organ without the target, the body contracted, an isodose volume. Everything is decided by integers and by comparisons of float32
 * values computed in the stated order, each rounded to float32, nothing contracted: the same inputs give the same bits across calls,
 * handles and processes, and tests/roi_ops_reference.py restates the rule in numpy.
 *
 * Inputs of a margin. An ROI A on a grid (nx, ny, nz); spacing_mm[3], positive and finite; margin_mm[6] in the order
 * (-x, +x, -y, +y, -z, +z) of the grid's index axes, every margin finite and >= 0.
 * Cost tables, one per axis a, made on the host in float64 from the float32 inputs: c_a[0] = 0; for d = 1, 2, ... on a side with
 *     margin m > 0: q = (double(d) * double(s_a)) / double(m), c = float(q * q); the table holds d while c <= 1.0f and ends at the
 *     first d where that fails. A side with m == 0 holds only d = 0. c_a[+d] uses the + margin, c_a[-d] the - margin. A side whose
 *     farthest d would exceed 127 refuses the call. (The rule is exact: at spacing float32(1.2) and margin 6, d = 5 is out, because
 *     the float32 spacing lies above 1.2 and the cost rounds above 1.)
 * Expand (contract == 0). A voxel p of the grid is in the result iff there is a q in A such that every component of d = p - q lies
 *     inside its table and fl32(fl32(c_x[d_x] + c_y[d_y]) + c_z[d_z]) <= 1.0f, the additions in exactly that order. The +x margin
 *     moves the +x surface outward; the element is an ellipsoid with a semi-axis of its own on each of the six sides.
 * Contract (contract == 1). p is in the result iff p is in A and no grid voxel q outside A has
 *     fl32(fl32(c_x[d_x] + c_y[d_y]) + c_z[d_z]) <= 1.0f for d = q - p inside the tables. The +x margin moves the +x surface inward.
 *     Voxels outside the grid count as inside A: the grid boundary does not erode a structure the grid cuts off. Equivalently: the
 *     complement within the grid of expand(complement of A within the grid, the two sides of every axis swapped), which is how it
 *     is computed.
 * The minimum over q separates exactly, because rounding is monotone:
 *     min_q fl(fl(c_x + c_y) + c_z) = min_dz fl(min_dy fl(min_dx c_x + c_y) + c_z);  the kernels (rtd_roi_ops.hpp) use this.
 *
 * rtd_roi_margin      expand or contract src. All margins zero (or below one spacing) give a copy.
 * rtd_roi_combine     op: RTD_ROI_OR, RTD_ROI_AND, RTD_ROI_ANDNOT (a without b), RTD_ROI_XOR; a and b of equal dims.
 * rtd_roi_from_mask   the voxels whose byte of dev_mask (device memory, dims[0] dims[1] dims[2] bytes, x fastest: the layout
 *                     rtd_roi_fill_mask writes) is non-zero.
 * All three are synchronous set-up calls like rtd_roi_rasterize (allocations, one wait for the total, the emit). Every result is a full
 * rtd_roi: rtd_roi_get_info, _voxels, _device, _fill_mask, _kernel_ms (the kernels of the call that made it) and _destroy work on it;
 * the list is strictly ascending, the box is the box of the voxels; n_planes and n_slices_covered describe contour input and are 0.
 * An empty result (a contraction that eats the structure, an AND of disjoint structures) is a valid ROI with n_voxels == 0. A result
 * may be an input again. The sources stay valid and unchanged.
 * Environment: RTD_ROI_MARGIN_NAIVE (read by rtd_create) selects the plain second implementation of the margin: one lane per voxel of
 * the working region, the nested table loops of the definition.
 *
 * RTD_ERR_INVALID_ARG, with *out = NULL, after which every object stays usable: a null pointer, a spacing that is not positive and
 * finite, a margin that is negative or not finite, a table side beyond 127, contract other than 0 or 1, an unknown op, ROIs of
 * different dims, a zero dimension or more than 2^31 - 1 voxels in rtd_roi_from_mask.
 */
#define RTD_ROI_OR     0
#define RTD_ROI_AND    1
#define RTD_ROI_ANDNOT 2   /* a without b */
#define RTD_ROI_XOR    3
int rtd_roi_margin(rtd_handle h, rtd_roi src, const float spacing_mm[3], const float margin_mm[6], int contract, rtd_roi* out);
int rtd_roi_combine(rtd_handle h, rtd_roi a, rtd_roi b, int op, rtd_roi* out);
int rtd_roi_from_mask(rtd_handle h, const uint32_t dims[3], const uint8_t* dev_mask, rtd_roi* out);

/*
 * ---- Dose volumes between grids: resampling through an index map, quantising for RT Dose ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). A dose that lives on another grid — another system's RT Dose file, a boost
 * plan, a previous course — is brought onto a destination grid through the affine map from destination voxel index to source voxel
 * index (rtd_dicom::idxToIdx, raytracedicom_amd.grids.index_map make it from the two index-to-world transforms), so that it can be
 * compared (rtd_dose_gamma wants one grid) or summed. The source is float32 or the quantised 16 / 32-bit pixels of an RT Dose file as
 * they stand; the destination is float32; both are x fastest, dims are (x, y, z), both live on the handle's device. Every operation
 * below is float32 in the stated order, each product, sum and difference rounded, nothing contracted: the same inputs give the same
 * bits across calls, handles and processes, and the rule can be restated in a few lines (tests/resample_reference.py does).
 *
 * Position. For destination voxel (x, y, z) and source axis a = 0, 1, 2, with (m, v) = dst_idx_to_src_idx and (n_0, n_1, n_2) = src_dims:
 *         p_a = ((m[3a] * float(x) + m[3a + 1] * float(y)) + m[3a + 2] * float(z)) + v[a]
 * Outside. The voxel is outside iff, for some a, not (p_a > -1.0f and p_a < float(n_a)); a NaN is outside. An outside voxel is written
 *     +0.0f, or left untouched when accumulate is set; nothing of the source is read for it.
 * Nodes. f_a = floorf(p_a), t_a = p_a - f_a; the nodes are f_a and f_a + 1 per axis. A node outside [0, n_a - 1] has the value +0.0f
 *     and is not read: the dose is zero beyond the grid it was computed on, so the result fades to zero over the last half voxel.
 *     A node inside has the value src[node] for RTD_DOSE_F32 and float(double(raw) * src_scale) for RTD_DOSE_U16 / RTD_DOSE_U32.
 * Blend. e = the trilinear blend of the 8 nodes, each blend a + t * (b - a) (one difference, one product, one sum), along x, then
 *     along y, then along z.
 * Output. out = scale * e;  dst[voxel] = out, or dst[voxel] + out when accumulate is set.
 * The map is only applied, never inverted: a singular one is legal. Source and destination must not overlap. dev_dst needs the
 * alignment of a float only (callers pass views into larger volumes).
 *
 * rtd_default_resample_options  RTD_DOSE_F32, no accumulation, scale 1, src_scale 1.
 * rtd_dose_resample             asynchronous on the handle's stream and launches only: no allocation, no copy, no host
 *                               synchronisation (it can be captured into a graph; a captured call is not timed).
 * rtd_dose_resample_kernel_ms   the time of the kernel of the handle's last rtd_dose_resample (hipEvents on the handle's stream; it
 *                               waits for that kernel), for reports. RTD_ERR_NOT_READY before any call.
 * RTD_ERR_INVALID_ARG, after which nothing has been written: a null pointer; a zero dimension or more than 2^31 - 1 voxels on either
 * side; an affine entry that is not finite; an unknown src_type; accumulate > 1; a scale that is not finite; an integer source with
 * src_scale not finite and > 0; a non-zero reserved word.
 *
 * rtd_dose_quantize             the write side of RT Dose: dev_dose (n_voxels floats) -> dev_out (n_voxels uint16 or uint32). Synchronous
 *                               (the scale is needed on the host). With *scaling_inout == 0 the scale is chosen: max = the largest
 *                               finite dose (from +0.0f; an integer atomicMax on the bit pattern), qmax = 2^bits - 1, s = the double
 *                               that strtod returns for the "%.10g" text of double(max) / qmax — the text an RT Dose writer stores as
 *                               DoseGridScaling, so that reader and writer agree on the double — and s = 1 when max == 0. (Ten
 *                               digits can round the quotient down by 5e-10 of itself, two steps at the top of 32 bits: while
 *                               rint(double(max) / s) > qmax the quotient is multiplied by 1 + 1e-10 and the text made again.) With
 *                               *scaling_inout > 0 that scale is used as given. On return *scaling_inout is the scale that was used.
 *                               q = rint(double(d) / s) in float64, ties to even; stored: 0 when q < 0 or d is a NaN, qmax when
 *                               q > qmax, q otherwise. *n_clamped (host, or NULL) = the number of voxels with not (0 <= q <= qmax):
 *                               the clamped ones and the NaNs, an integer count. The first call allocates 16 bytes on the device.
 * RTD_ERR_INVALID_ARG: a null h, dev_dose, scaling_inout or dev_out; n_voxels == 0; bits other than 16 and 32; a scaling that is
 * negative or not finite.
 *
 * Kernel (rtd_resample.hpp): one lane per destination voxel, lanes along x; the outside test precedes every load; the destination is
 * written once with non-temporal stores, which leaves the caches to the source nodes that neighbouring lanes and rows share.
 */
enum { RTD_DOSE_F32 = 0, RTD_DOSE_U16 = 1, RTD_DOSE_U32 = 2 };
typedef struct rtd_resample_options {
    uint32_t src_type;     /* RTD_DOSE_* */
    uint32_t accumulate;   /* 0: dst[v] = out; 1: dst[v] = dst[v] + out, voxels outside the source untouched */
    float    scale;        /* 1.0: out = scale * e */
    uint32_t reserved0;    /* zero */
    double   src_scale;    /* DoseGridScaling of an integer source; ignored for RTD_DOSE_F32 */
    uint32_t reserved[2];  /* zero */
} rtd_resample_options;    /* 32 bytes */
void rtd_default_resample_options(rtd_resample_options* out);
int rtd_dose_resample(rtd_handle h, const void* dev_src, const uint32_t src_dims[3], const rtd_affine* dst_idx_to_src_idx,
                      float* dev_dst, const uint32_t dst_dims[3], const rtd_resample_options* opt);
int rtd_dose_resample_kernel_ms(rtd_handle h, float* ms);   /* as rtd_dose_gamma_kernel_ms */
int rtd_dose_quantize(rtd_handle h, const float* dev_dose, size_t n_voxels, int bits /* 16 | 32 */,
                      double* scaling_inout /* in: > 0 use it, 0 choose; out: the one used */,
                      void* dev_out /* uint16 or uint32 [n_voxels] */, uint64_t* n_clamped /* host, may be NULL */);

/*
 * ---- Deformable dose warping: a dose through a displacement field, and the transposed operation ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; rtd_dose_resample and rtd_resample_options are untouched). A dose computed on
 * one anatomy — a breathing phase, the CT of the day, a previous course — is pulled onto a reference anatomy through a deformation
 * vector field (DVF): for every voxel of the destination (reference) grid the field gives the displacement that leads to the matching
 * place of the source anatomy. rtd_dose_warp is rtd_dose_resample with that displacement added to the position; rtd_dose_warp_t is its
 * transpose, which pushes a voxel gradient on the reference grid back to the source grid (where Dij^T lives). All volumes are x
 * fastest, dims are (x, y, z), everything lives on the handle's device. Every operation is float32 in the stated order, each product,
 * sum and difference rounded, nothing contracted (tests/warp_reference.py restates both rules in numpy).
 *
 * rtd_warp: dst_idx_to_src_idx as rtd_dose_resample takes it; dst_idx_to_dvf_idx, destination voxel index -> node index of the field's
 * grid; disp_to_src_idx = k, row-major 3 x 3, displacement vector (for instance mm) -> source-index units; dev_dvf, component-major:
 * three volumes of dvf_dims voxels, component 0, then 1, then 2; reserved words zero. raytracedicom_amd.grids.warp_maps makes the three
 * maps from the index-to-world transforms of the three grids.
 *
 * Forward, rtd_dose_warp(h, dev_src, src_dims, warp, dev_dst, dst_dims, opt), opt as for rtd_dose_resample (src_type, scale, src_scale,
 * accumulate mean what they mean there). For destination voxel (x, y, z):
 * Field position. q_a = the Position formula of rtd_dose_resample with (m, v) = dst_idx_to_dvf_idx, a = 0, 1, 2. If a q_a is a NaN the
 *     voxel is outside. Otherwise, with (n_0, n_1, n_2) = dvf_dims: qc_a = fminf(fmaxf(q_a, 0), float(n_a - 1)) — the field is held
 *     constant beyond its grid —, i0_a = (int)floorf(qc_a), i1_a = min(i0_a + 1, n_a - 1), t_a = qc_a - floorf(qc_a). A dimension of 1
 *     is legal.
 * Displacement. For each component c, u_c = the trilinear blend of the 8 field nodes (i0 | i1 per axis) of volume c, each blend
 *     a + t * (b - a), along x, then y, then z.
 * Position. s_a = (k[3a] * u_0 + k[3a + 1] * u_1) + k[3a + 2] * u_2;  p_a = P_a + s_a, where P_a is rtd_dose_resample's p_a for
 *     dst_idx_to_src_idx.
 * From here on rtd_dose_resample's rule holds word for word: Outside, Nodes, Blend, Output. A displacement that is not finite makes
 *     p_a a NaN (or infinite): the voxel is outside.
 * With an all-zero field the result is bit for bit that of rtd_dose_resample with the same map (a position of -0.0 becomes +0.0, which
 * changes no result). The call is asynchronous on the handle's stream and launches only (no allocation, no copy, no host
 * synchronisation; it can be captured, and a captured call is not timed). rtd_dose_warp_kernel_ms: the time of the kernel of the
 * handle's last rtd_dose_warp, as rtd_dose_resample_kernel_ms. RTD_ERR_INVALID_ARG, after which nothing has been written: everything
 * rtd_dose_resample refuses (the dimensions of the field count as a third grid), a null warp or dev_dvf, an entry of k or of either
 * affine that is not finite, a non-zero reserved word of the record.
 *
 * Transpose, rtd_dose_warp_t(h, dev_g_dst, dst_dims, warp, dev_g_src, src_dims, scale, accumulate, dev_workspace, workspace_bytes):
 * float32 only. g_src = scale * W^T g_dst, where W is the forward operator of a float32 source at scale 1. A scatter: float sums
 * would depend on the order in which the atomics arrive, so the sums are 64-bit integers of a quantum, which are associative.
 * Per destination voxel. sg = scale * g_dst[voxel]; an sg that is not finite counts as zero everywhere below.
 * Maximum. M = max |sg| over the destination (on the device: an integer atomicMax on the bit pattern). M == 0: the result is +0.0f in
 *     every source voxel, or dev_g_src is left as it is when accumulate is set. Otherwise M = m * 2^E with m in [0.5, 1), and the
 *     quantum is 2^(E - 30).
 * Contribution. For a voxel the forward rule calls inside, with f_a, t_a of Nodes: w0_a = 1.0f - t_a, w1_a = t_a; its contribution to
 *     node (dx, dy, dz) is c = ((sg * wx) * wy) * wz. A node outside [0, n_a - 1] receives nothing.
 * Accumulation. S_j += llrint(double(c) * 2^(30 - E)), ties to even, into one int64 per source voxel (64-bit integer atomics on the
 *     workspace). The scaling by a power of two is exact; |c| <= M < 2^E bounds every term by 2^30 and there are fewer than 2^31
 *     terms, so no sum overflows; each contribution is off by at most half a quantum, which is at most M * 2^-30.
 * Finish. out_j = float(double(S_j) * 2^(E - 30));  g_src[j] = out_j, or g_src[j] + out_j when accumulate is set — for every source
 *     voxel j.
 * rtd_dose_warp_t_workspace_bytes(src_dims, &bytes): 64 bytes of header plus one int64 per source voxel. The caller owns the workspace
 * (8-byte aligned, its content on entry is irrelevant), so the call allocates nothing and can be captured: a memset of the workspace,
 * then the maximum, scatter and finish kernels on the handle's stream. rtd_dose_warp_t_kernel_ms: the times of those four launches of
 * the last call that was not captured. RTD_ERR_INVALID_ARG, after which nothing has been written: as for rtd_dose_warp, a scale that
 * is not finite, accumulate > 1, a null or misaligned workspace, workspace_bytes below the size above.
 *
 * Kernels (rtd_warp.hpp): forward and scatter are one lane per destination voxel, lanes along x, the block of rtd_dose_resample. The
 * scatter merges within a block before its atomics go out: a block takes 64 x 4 x 4 destination voxels, whose contributions under
 * the near-identity maps of real registrations fall into a box of source nodes little larger than that; it sums them in an LDS tile
 * of 72 x 7 x 8 int64 and sends one global atomic per tile node that is not zero (a voxel whose nodes leave the tile sends its own).
 * The integers are summed exactly either way: the bits do not depend on it (RTD_WARP_T_PLAIN in the environment when the handle is
 * created selects the scatter with eight global atomics per voxel, for measurements).
 */
typedef struct rtd_warp {
    rtd_affine   dst_idx_to_src_idx;   /* offset   0 */
    rtd_affine   dst_idx_to_dvf_idx;   /* offset  48 */
    float        disp_to_src_idx[9];   /* offset  96: k, row-major */
    uint32_t     reserved0;            /* offset 132: zero */
    const float* dev_dvf;              /* offset 136: [3][dvf_dims z][y][x] on the device */
    uint32_t     dvf_dims[3];          /* offset 144: (x, y, z) */
    uint32_t     reserved[5];          /* offset 156: zero */
} rtd_warp;    /* 176 bytes */
int rtd_dose_warp(rtd_handle h, const void* dev_src, const uint32_t src_dims[3], const rtd_warp* warp, float* dev_dst,
                  const uint32_t dst_dims[3], const rtd_resample_options* opt);
int rtd_dose_warp_kernel_ms(rtd_handle h, float* ms);
int rtd_dose_warp_t_workspace_bytes(const uint32_t src_dims[3], size_t* bytes);
int rtd_dose_warp_t(rtd_handle h, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warp, float* dev_g_src,
                    const uint32_t src_dims[3], float scale, uint32_t accumulate, void* dev_workspace, size_t workspace_bytes);
int rtd_dose_warp_t_kernel_ms(rtd_handle h, float ms[4] /* memset, maximum, scatter, finish */);

/*
 * ---- 4D dose: phases warped and summed, and an optimiser on the accumulated dose ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel result or structure above changes). A 4D plan is
 * judged on the dose accumulated over the breathing phases of a 4DCT: every phase's dose pulled onto one reference anatomy through
 * that phase's deformation field and summed with the time spent in the phase as its weight. The two calls below are the warps of the
 * block above over a phase axis; rtd_optimizer_create_4d puts them into the resident iteration. All phases share one source grid,
 * src_dims (the phases of a 4DCT do); sources are float32; 1 <= n <= RTD_4D_MAX_PHASES.
 *
 * rtd_dose_warp_sum(h, dev_srcs, src_dims, warps, weights, n, dev_dst, dst_dims): dev_srcs a HOST array of n device pointers, warps host
 * rtd_warp[n], weights host float[n], each finite. The result is bit for bit what these calls give in order:
 * rtd_dose_warp(src_0, warp_0, dst, scale = weights[0], accumulate = 0), then rtd_dose_warp(src_p, warp_p, dst, scale = weights[p],
 * accumulate = 1) for p = 1 .. n - 1. Per destination voxel: d = inside_0 ? weights[0] * e_0 : 0.0f, then for ascending p,
 * if (inside_p) d = d + weights[p] * e_p, with inside_p and e_p the forward rule's for phase p; every product and sum is rounded on
 * its own. One launch writes the destination once (non-temporal); nothing is read back. It launches only and can be captured.
 * RTD_ERR_INVALID_ARG, after which nothing has been written: whatever rtd_dose_warp refuses of a phase, n of 0 or above 16, a null
 * array or a null entry of dev_srcs, a weight that is not finite.
 *
 * rtd_dose_warp_t_phases(h, dev_g_dst, dst_dims, warps, weights, n, dev_g_srcs, src_dims, dev_workspace, workspace_bytes):
 * dev_g_srcs[p] (a HOST array of n device pointers) gets, bit for bit, what rtd_dose_warp_t(g, warp_p, scale = weights[p],
 * accumulate = 0) writes. rtd_dose_warp_t_phases_workspace_bytes(src_dims, n, &bytes): n times rtd_dose_warp_t_workspace_bytes; slice p
 * begins at p times the single call's size and keeps its own 64-byte header. Four operations in all on the handle's stream: one
 * memset of the whole workspace, one maximum kernel that reads g once and keeps n maxima M_p = max |weights[p] * g| (each phase's own
 * products: a product that overflows counts as zero, as the rule above says, so M_p is NOT weights[p] times one max |g|), one scatter
 * kernel and one finish kernel with the phase on the grid. RTD_WARP_T_PLAIN keeps its meaning; the bits are the same. Refusals as
 * rtd_dose_warp_t's per phase, and those of the arrays as above. It launches only and can be captured.
 *
 * rtd_optimizer_create_4d(h, fields, n_fields, fourd, obj, options, &opt): fields is [n_phases][n_fields], phase-major: a phase is a
 * row of fields, the same beams computed on that phase's CT, each with its matrix. All phases carry ONE weight vector; the spot-map
 * shape of field f must equal that of phase 0's field f; all fields share one dose grid, the phase grid. The objective lives on the
 * reference grid, whose dims may differ from the phase grid's. warps[p] leads from a reference voxel to phase p's dose grid (what
 * rtd_dose_warp takes with src_dims = the phase grid and dst_dims = the objective's dims); the records are copied, dev_dvf stays the
 * caller's: THE FIELDS MUST OUTLIVE THE OPTIMISER. weights[p] (finite, > 0: the time spent in the phase) is used as given; NULL:
 * float(1.0 / n_phases) each. The call returns an ordinary rtd_optimizer: rtd_optimizer_set_weights, _run, _result, _weights and
 * _destroy work on it unchanged; the start weights are phase 0's.
 * One iteration, launches on the handle's stream only, no decision on the host, capturable:
 *   1. dose_p = sum_f Dij_{p,f} w_f into P volumes on the phase grid (the batched products of the robust optimiser);
 *   2. acc = sum_p a_p W_p dose_p on the reference grid: rtd_dose_warp_sum's launch;
 *   3. rtd_objective_eval(acc): f, the term values and g on the reference grid (every term kind of the plain optimiser, DVH and EUD
 *      terms included);
 *   4. g_p = a_p W_p^T g: rtd_dose_warp_t_phases's four operations on a workspace the optimiser owns;
 *   5. grad_p = Dij_{p,f}^T g_p per field (the batched transposed products, every phase taken);
 *   6. grad[j] = float32(sum_p double(grad_p[j])), p ascending, the sum starting from the first term, rounded once (the phase
 *      weights already act through the warps' scale);
 *   7. steps 4 to 7 of the plain iteration, word for word.
 * rtd_optimizer_dose answers acc of the iterate that entered the last iteration, rtd_optimizer_scenario_dose(p) dose_p;
 * rtd_optimizer_scenario_values answers as for a composite: f_p = f_last for every p, lambda 1.0, worst 0.
 * Memory: per phase a dose volume, a g volume and a workspace slice, 16 bytes per phase-grid voxel per phase (4.3 GB at 256^3 and 16
 * phases), plus acc and g on the reference grid. A failed allocation is RTD_ERR_OUT_OF_MEMORY with everything freed.
 * RTD_4D_NO_BATCH in the environment at creation makes the optimiser issue the per-phase public sequences instead (rtd_dose_warp P
 * times, rtd_dose_warp_t P times each on its slice, the unbatched products): the same bits, for tests and measurements.
 * The optimiser notes every field's matrix at creation; rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before its first launch,
 * once rtd_field_dose_influence has been called again on one of the fields: destroy the optimiser and create a new one.
 * RTD_ERR_INVALID_ARG: whatever rtd_optimizer_create_robust refuses of a field list; n_phases of 0 or above 16; a null warps; a warp
 * that rtd_dose_warp would refuse between the phase grid and the objective's dims; a weight that is not finite and positive; a
 * non-zero reserved word. RTD_ERR_NOT_READY: a field without a matrix. rtd_optimizer_set_let_objective and rtd_optimizer_set_rbe
 * refuse a 4D optimiser as they refuse a robust one. After a refusal every object stays usable.
 *
 * Out of scope: phases combined with set-up or range scenarios; the voxel-wise worst case over phases; LET and RBE; phases on
 * different dose grids; a forward sum restricted to the ROI union; energy- or mass-conserving warps; a registration reader;
 * nuclear_corr, remote fields and the rtd_plan_* path; interplay with the delivery time structure.
 */
enum { RTD_4D_MAX_PHASES = 16 };
int rtd_dose_warp_sum(rtd_handle h, const float* const* dev_srcs, const uint32_t src_dims[3], const rtd_warp* warps, const float* weights,
                      uint32_t n, float* dev_dst, const uint32_t dst_dims[3]);
int rtd_dose_warp_t_phases_workspace_bytes(const uint32_t src_dims[3], uint32_t n, size_t* bytes);
int rtd_dose_warp_t_phases(rtd_handle h, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warps, const float* weights,
                           uint32_t n, float* const* dev_g_srcs, const uint32_t src_dims[3], void* dev_workspace, size_t workspace_bytes);
typedef struct rtd_4d_options {
    uint32_t n_phases;          /* 1 .. RTD_4D_MAX_PHASES */
    uint32_t reserved0;
    const rtd_warp* warps;      /* [n_phases]: reference voxel -> phase p's dose grid; the records are copied, dev_dvf stays the caller's */
    const float* weights;       /* [n_phases], finite and > 0 (time spent in the phase), used as given; NULL: float(1.0 / n_phases) each */
    int32_t reserved[4];
} rtd_4d_options;               /* 40 bytes */
int rtd_optimizer_create_4d(rtd_handle h, const rtd_field* fields /* [n_phases][n_fields], phase-major */, uint32_t n_fields,
                            const rtd_4d_options* fourd, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);

/*
 * ---- Dose-averaged LET: the LET-weighted influence matrix, LETd, a LET objective ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). The convention is the analytical one: the LET of spot j at voxel v is the
 * LET of that spot's energy at the voxel's water-equivalent depth along the field. With D the field's dose-influence matrix, the
 * LET-weighted matrix is N[v][j] = float32(D[v][j] * L(l(j), depth[v])) on the SAME sparsity structure; N w is the LET-weighted dose
 * (keV/um x dose unit, matRad's mLETDose) and LETd = (sum_f N_f w_f) / (sum_f D_f w_f) voxel by voxel. Every rule below is float32 in
 * the stated order, nothing contracted; tests/let_reference.py restates them in numpy.
 *
 * rtd_set_let_table        the table [n_energies][n_energy_samples] float32 in keV/um: the rows of energies_per_u and the depth
 *                          sampling of cidd_matrix (sample index = depth in mm * scale_facts[e]). Copied into a device allocation of
 *                          its own. It is not an input of the dose: nothing a compute reuses is invalidated. RTD_ERR_INVALID_ARG when
 *                          the LUTs are not set, the dimensions differ from the handle's LUTs, or an entry is not finite or is negative.
 *                          NULL removes the table. Synchronous. A field's LET values belong to the table they were made from: after a
 *                          new table the products answer RTD_ERR_NOT_READY until rtd_field_let_influence has run again.
 * rtd_field_water_depth    WRITES, for every voxel of the field's dose box (the box rtd_field_clear_dose clears) and nothing outside it,
 *                          the field's water-equivalent depth at the voxel in mm into dev_depth (a volume on the field's dose grid).
 *     Position. p = getFanIdx of the field's transfer parameters at the voxel (what the transfer samples the BEV dose at), moved into
 *         the indices of the [S][H][W] trace arrays: i = p.x - 32.0f, j = p.y - 32.0f, k = p.z + float(beam_first_inside).
 *     Depth of trace sample (k, j, i). 0.5f * (wepl[k] + old), old = wepl[k - 1] for k > beam_first_inside and 0 otherwise: the
 *         mid-point of the cumulative depth before and after the step, where the fill deposits the step's dose.
 *     Blend. Per axis with extent n: a position that is not >= 0 takes node 0, one >= n - 1 node n - 1, both with weight 0 (CLAMP at
 *         all six faces; a voxel behind the last step takes the last depth); otherwise nodes floorf(p), floorf(p) + 1 and weight
 *         a = p - floorf(p). Each blend is (1 - a) * v0 + a * v1, along x, then y, then z.
 *                          One launch on the handle's stream, no allocation, no synchronisation. RTD_ERR_NOT_READY before any compute
 *                          of the field; RTD_ERR_INVALID_ARG for a remote field, nuclear_corr or a null pointer. It writes nothing a
 *                          later transfer, gradient or Dij call reads.
 * rtd_field_let_influence  computes N for the matrix of the field's last rtd_field_dose_influence (rtd_field_dose_influence_prepare runs
 *                          first where it has not): the depth above over the matrix's row box, then one values array for the CSC and
 *                          one for the row-major companion by the same expression (a voxel has one depth and a column one layer: the
 *                          two hold the same bits; 4 bytes per entry each, no new index arrays).
 *     Table. L(l, d): rows floor(energyIdx_l) and the next one, clamped to the table, with the fill's row weight
 *         energyIdx_l - floor(energyIdx_l); within a row the position d * energyScaleFact_l clamped to [0, n_samples - 1] (a NaN to
 *         0), nodes floor and the next, blends as above: first inside each row, then between the rows.
 *                          Launches only once its three buffers exist (the first call after a new matrix allocates them).
 *                          RTD_ERR_NOT_READY without a matrix or without a table; RTD_ERR_OUT_OF_MEMORY when the allocation fails (the
 *                          matrix stays usable). The values live with the matrix: a new rtd_field_dose_influence discards them, release
 *                          or destroy frees them. It uses the trace of the field's last compute.
 * rtd_field_let_influence_apply / _apply_t   N w and N^T g: the kernels of rtd_field_dose_influence_apply / _apply_t launched with the
 *                          LET values: their summation trees, the init semantics and the box are those. Launches only.
 *                          RTD_ERR_NOT_READY before rtd_field_let_influence (of the current matrix and table).
 * rtd_field_let_influence_device   the device pointer of the CSC LET values; the indices are those of rtd_field_dose_influence_device.
 * rtd_let_average          out[v] = dose[v] > dose_floor ? let_dose[v] / dose[v] : 0 (a float32 division): LETd. One launch; in place on
 *                          either input is allowed. RTD_ERR_INVALID_ARG for a null pointer or a dose_floor that is not >= 0.
 * rtd_optimizer_set_let_objective   a second objective on the same dose grid for a plain optimiser, evaluated on the volume
 *                          sum_f N_f w_f: its ROIs and terms are ordinary ones, so an over-dose term on an organ at risk is a cap on
 *                          LET x D there. Per iteration the LET-weighted dose is formed the way the dose is, both objectives are
 *                          evaluated, f = f_dose + f_let in float64, Dij^T g_dose and N^T g_let are computed separately and
 *                          grad = float32(a + b) per entry in that order; everything after that is unchanged. The optimiser owns one
 *                          more dose volume, one more g volume and one more gradient vector, allocated in this call, never in
 *                          rtd_optimizer_run, which stays launches-only and capturable. The objective must outlive its use and be an
 *                          object other than the optimiser's own. RTD_ERR_NOT_READY unless every field has its LET matrix;
 *                          RTD_ERR_INVALID_ARG for a robust or voxel-wise optimiser, other dims or an objective without terms. NULL
 *                          removes it (synchronous): without one the optimiser's bits are what they are without this block.
 * rtd_optimizer_let_dose   the LET-weighted dose volume of the last iteration (owned by the optimiser).
 * rtd_optimizer_let_values [f, f_dose, f_let] of the last iteration (synchronous). Both RTD_ERR_NOT_READY without a LET objective.
 *
 * Out of scope: LET through the rtd_plan_* path, with nuclear_corr or for remote fields (refused as the matrix itself refuses them);
 * LET objectives in the robust and voxel-wise optimisers; a command-line flag; a file format for LET tables; variable-RBE models (a
 * caller builds them voxel-wise from LETd and dose).
 */
enum { RTD_ERR_OUT_OF_MEMORY = -7 };   /* a device allocation failed and the call says what stays usable */
int rtd_set_let_table(rtd_handle h, const float* let_matrix, int32_t n_energies, int32_t n_energy_samples);
int rtd_field_water_depth(rtd_handle h, rtd_field f, float* dev_depth);
int rtd_field_let_influence(rtd_handle h, rtd_field f);
int rtd_field_let_influence_apply(rtd_handle h, rtd_field f, const float* dev_w, float* dev_out, int init);
int rtd_field_let_influence_apply_t(rtd_handle h, rtd_field f, const float* dev_g, float* dev_spot_grad);
int rtd_field_let_influence_device(rtd_handle h, rtd_field f, const float** values, size_t* nnz);
int rtd_let_average(rtd_handle h, const float* dev_let_dose, const float* dev_dose, size_t n_voxels, float dose_floor, float* dev_out);
int rtd_optimizer_set_let_objective(rtd_handle h, rtd_optimizer opt, rtd_objective let_objective);
int rtd_optimizer_let_dose(rtd_handle h, rtd_optimizer opt, const float** dev);
int rtd_optimizer_let_values(rtd_handle h, rtd_optimizer opt, double values[3]);

/*
 * ---- Variable-RBE dose: LQ models on dose and LETd, resident in the optimiser ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3). Proton plans are prescribed in RBE-weighted dose. For every LQ model whose
 * RBEmax and RBEmin are lines in LETd (McNamara, Wedenberg, Carabe, the constant 1.1) the biological effect is a quadratic in two
 * volumes that exist on the device: d = sum_f Dij_f w_f, the dose, and n = sum_f N_f w_f, the LET-weighted dose of the block above
 * (n = LETd * d). The interface knows no model names. A tissue class carries the photon parameters alpha_x (1/Gy) and beta_x (1/Gy^2)
 * and the two lines RBEmax = rbe_max[0] + rbe_max[1] * LETd, RBEmin = rbe_min[0] + rbe_min[1] * LETd; with alpha = alpha_x * RBEmax
 * and sqrt(beta) = sqrt(beta_x) * RBEmin:
 *
 *     A = a0*d + a1*n          a0 = alpha_x*rbe_max[0]        a1 = alpha_x*rbe_max[1]
 *     B = b0*d + b1*n          b0 = sqrt(beta_x)*rbe_min[0]   b1 = sqrt(beta_x)*rbe_min[1]
 *     e = A + B*B                                   (biological effect)
 *     s = sqrt(alpha_x*alpha_x + (4*beta_x)*e)
 *     R = (2*e) / (s + alpha_x)                     (RBE-weighted dose; this form does not cancel at small e)
 *     k = 1 / s                                     (dR/de)
 *     fd = k * (a0 + (2*B)*b0)                      (dR/dd)
 *     fn = k * (a1 + (2*B)*b1)                      (dR/dn)
 *
 * The host forms a0 .. b1 in float64 from the float fields of the tissue (sqrt(beta_x) in float64) and rounds each once to float32.
 * Everything per voxel is float32 in exactly the order written, nothing contracted; the division and the square root are the correctly
 * rounded ones. A voxel whose e is not >= 0 (a negative or NaN input) gives R = 0, fd = 0, fn = 0. e == 0 takes the formulas (R = 0,
 * k = 1/alpha_x): a voxel that starts without dose still has a gradient. Backward: g_d[v] = g_R[v] * fd, g_n[v] = g_R[v] * fn.
 * tests/rbe_reference.py restates all of it in numpy; raytracedicom_amd/rbe.py has the four named models.
 *
 * rtd_rbe_create           an object on a dose grid: one uint8 class per voxel (class 0, default_tissue, everywhere) and a table of at
 *                          most 256 x 6 floats; no per-voxel coefficient volumes. Synchronous.
 * rtd_rbe_add_tissue       one more class; class_id receives 1 .. 255. Synchronous.
 * rtd_rbe_assign_voxels    the class of a list of linear voxel indices ((z ny + y) nx + x, any order). Synchronous.
 * rtd_rbe_assign_roi       the class of an ROI's voxels, from its resident list (no copy to the host): one launch on the handle's stream.
 *                          A later assignment overwrites an earlier one: that is the priority rule for overlapping structures.
 * rtd_rbe_classes_device   the device pointer of the class volume (owned by the object).
 * rtd_rbe_dose             WRITES R of the voxels of box (inclusive min[3], max[3], as dose_box_min / dose_box_max; NULL: the grid)
 *                          into dev_rbe_dose; voxels outside the box are not touched. dev_rbe_dose may be dev_dose or dev_let_dose.
 * rtd_rbe_backward         WRITES g_d and g_n of the voxels of box. dev_g_dose and dev_g_let must be two volumes; either may be any of
 *                          the three inputs (a voxel's outputs depend on that voxel only, and it is read before it is written).
 *                          Both: one launch on the handle's stream, no allocation, no synchronisation.
 *                          The RBE factor R / d needs no call of its own: rtd_let_average(R, d, floor) is the same division.
 * rtd_rbe_destroy          waits for the stream and frees the object. It must outlive its use by an optimiser.
 * rtd_optimizer_set_rbe    a plain optimiser then evaluates its objective on R instead of d. Allocated in this call, never in
 *                          rtd_optimizer_run: the n volume, the R volume, the g_R volume, the g_n volume and a second gradient vector;
 *                          the union of the fields' matrix row boxes is computed once, and everything outside it stays at the zero it
 *                          was allocated with. An iteration: d = sum_f Dij_f w_f and n = sum_f N_f w_f as in the block above;
 *                          rtd_rbe_dose on the box; the objective on R, which gives g_R; rtd_rbe_backward on the box into g_d and g_n;
 *                          Dij^T g_d and N^T g_n; grad = float32(a + b) per entry in that order; everything after that is unchanged.
 *                          rtd_optimizer_run stays launches-only and capturable, and refuses (RTD_ERR_NOT_READY, before its first
 *                          launch) when a field's LET values are not those of its matrix and the handle's table. RTD_ERR_NOT_READY
 *                          unless every field has its LET matrix; RTD_ERR_INVALID_ARG for a robust or voxel-wise optimiser, for an
 *                          object on other dims, and when the optimiser has a LET objective (rtd_optimizer_set_let_objective likewise
 *                          refuses an optimiser that has an RBE model: one or the other). NULL removes it (synchronous): the
 *                          optimiser's bits are then those of one that never had one. rtd_optimizer_dose keeps returning d.
 * rtd_optimizer_rbe_dose   the R volume of the last iteration (owned by the optimiser); RTD_ERR_NOT_READY without a model.
 *
 * RTD_ERR_INVALID_ARG: a null pointer; a zero dimension or more than 2^31 - 1 voxels; alpha_x or beta_x not finite or not > 0; a
 * non-finite line coefficient; non-zero reserved words; an unknown class; a voxel index outside the grid; an ROI on other dims; a box
 * outside the grid or with min > max; a 257th class. After a refusal nothing has been written and every object stays usable.
 *
 * Out of scope: RBE in the robust and voxel-wise optimisers; RBE together with a LET objective; the rtd_plan_* path, nuclear_corr and
 * remote fields (refused as the matrix itself refuses them); per-voxel alpha_x / beta_x maps; models that are not linear in LETd; a
 * command-line flag.
 */
typedef struct rtd_rbe_tissue {
    float alpha_x, beta_x;    /* photon LQ parameters, 1/Gy and 1/Gy^2 */
    float rbe_max[2];         /* RBEmax = rbe_max[0] + rbe_max[1] * LETd (LETd in keV/um) */
    float rbe_min[2];         /* RBEmin = rbe_min[0] + rbe_min[1] * LETd */
    uint32_t reserved[2];     /* zero */
} rtd_rbe_tissue;             /* 32 bytes */
typedef struct rtd_rbe_s* rtd_rbe;
int rtd_rbe_create(rtd_handle h, const uint32_t dose_dims[3], const rtd_rbe_tissue* default_tissue, rtd_rbe* out);
int rtd_rbe_add_tissue(rtd_handle h, rtd_rbe rbe, const rtd_rbe_tissue* tissue, int32_t* class_id);
int rtd_rbe_assign_voxels(rtd_handle h, rtd_rbe rbe, const int32_t* host_voxels, size_t n, int32_t class_id);
int rtd_rbe_assign_roi(rtd_handle h, rtd_rbe rbe, rtd_roi roi, int32_t class_id);
int rtd_rbe_classes_device(rtd_handle h, rtd_rbe rbe, const uint8_t** dev_classes);
int rtd_rbe_dose(rtd_handle h, rtd_rbe rbe, const float* dev_dose, const float* dev_let_dose, const int32_t box[6], float* dev_rbe_dose);
int rtd_rbe_backward(rtd_handle h, rtd_rbe rbe, const float* dev_dose, const float* dev_let_dose, const float* dev_g_rbe, const int32_t box[6],
                     float* dev_g_dose, float* dev_g_let);
int rtd_rbe_destroy(rtd_handle h, rtd_rbe rbe);
int rtd_optimizer_set_rbe(rtd_handle h, rtd_optimizer opt, rtd_rbe rbe);
int rtd_optimizer_rbe_dose(rtd_handle h, rtd_optimizer opt, const float** dev);

/*
 * ---- Plan sets: P plans optimised at once over one resident matrix ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel or structure above changes). Nobody plans with one
 * optimiser run: the anchor plans and the balanced plan of a Pareto navigation, the sweep of a penalty, a set of prescription levels
 * are plans on the same fields and structures whose terms differ in weight and level alone. A plan set iterates P weight vectors
 * under P variants of one objective; every step of the iteration is ONE launch for all plans, built on the two products with P
 * right-hand sides (rtd_field_dose_influence_apply_set / _apply_t_set), so the matrix is read twice per iteration whatever P is.
 *
 * THE CONTRACT. For every plan p take a plain rtd_optimizer on the same fields, with a plain objective of the same ROIs and the
 * terms variants[p], started from the same weights. After the same number of iterations, however they are split over runs, these
 * are equal BIT FOR BIT between plan p and that optimiser: w, w_best, the dose volume, every field of the report (f_last, f_best,
 * step, best_iteration, iterations, history_len, guarded) and the history. Everything follows the text of the plain iteration,
 * steps 1 to 7 above, per plan: c_t and wn_t of a variant are computed on the host in float64 exactly as rtd_objective_add_term's are;
 * the float64 trees of the evaluation and of the step length are the plain ones; the update rounds float32(alpha_p) * grad before
 * the subtraction; the guard is per plan: a plan whose objective is not finite goes back to its own w_best and forgets its own
 * Barzilai-Borwein pair, and the other plans do not notice.
 *
 * rtd_planset_create       obj supplies the ROIs and the term structure; variants[p * n_terms + t] is term t as plan p sees it: the
 *                          kind and roi of the objective's term t, its own weight (> 0, finite) and dose_level (finite). 1 <= n_plans
 *                          <= RTD_PLANSET_MAX_PLANS. options as rtd_optimizer_create (NULL: the defaults; every plan has its own
 *                          history of history_capacity entries). Every plan's w and w_best start as each field's own spot weights.
 *                          Runs rtd_field_dose_influence_prepare where it has not run. Synchronous. The fields, their matrices and
 *                          the objective must outlive the set unchanged. rtd_planset_run refuses, RTD_ERR_NOT_READY and before its
 *                          first launch, once a term or an ROI has been added to the objective (evaluated again since or not, with or
 *                          without terms on the new ROI) or rtd_field_dose_influence has been called again on one of the fields,
 *                          prepared or not: the set's buffers are sized for the objective and the matrices it was created on. Such
 *                          a set can only be destroyed; create a new one.
 *                          Memory the set owns, at plan_stride = n_plans rounded up to 1, 2, 4, 8 or 16: the dose and the g volume,
 *                          plan-minor, 8 * plan_stride bytes per dose-grid voxel together; the five vectors, 20 * plan_stride bytes
 *                          per spot; 4 * plan_stride bytes per column chunk of the field with the most; 8 * plan_stride bytes per
 *                          (term, block of 256 union voxels); the histories and a few records.
 * rtd_planset_set_weights  dev_w: [L][ny][nx] float32, contiguous, of field field_index; copied on the stream into plan `plan`'s w
 *                          (before the first run into its w_best too), as rtd_optimizer_set_weights.
 * rtd_planset_run          launches n_iterations iterations of every plan; launches only (no allocation, no copy, no host
 *                          synchronisation, no decision on the host: a run can be captured into a graph). The launches of one
 *                          iteration, their number independent of n_plans: the clear of the row box of every field but the first;
 *                          apply_set per field (field 0 with init = 1); the evaluation and its reduction; apply_t_set and its reduce
 *                          per field; partials, step, update.
 * rtd_planset_result       rtd_optimizer_result of plan `plan` (waits for the stream; RTD_ERR_INVALID_ARG with the report filled when
 *                          that plan's start was not finite).
 * rtd_planset_weights      plan `plan`'s w (best == 0) or w_best of field field_index, de-interleaved to dev_w_out (contiguous).
 * rtd_planset_dose         plan `plan`'s dose volume (of the iterate that entered the last iteration), copied out of the interleaved
 *                          one into dev_dose_out (contiguous, the whole grid). Asynchronous.
 * rtd_planset_values       waits; values_out: host float64 [n_plans][1 + n_terms]: per plan the objective and the value of every
 *                          term of the iterate that entered the last iteration: the bits of rtd_objective_eval of the plain objective
 *                          with that plan's terms on rtd_planset_dose(plan). The trade-off table a navigation reads.
 * rtd_planset_blend        dev_w_out[j] = float32(sum over p ascending, from 0.0, of coeffs[p] * double(w_p[j])) for the spots of field
 *                          field_index, w_p plan p's w_best (best != 0) or w; float64, no contraction, rounded once. coeffs: host
 *                          float64 [n_plans], finite and >= 0. The dose is linear in w and w >= 0 is kept: this is the navigated plan,
 *                          and its dose is one rtd_field_dose_influence_apply per field.
 * rtd_planset_destroy      frees it (before its fields, its objective and its handle).
 *
 * RTD_ERR_INVALID_ARG: what rtd_optimizer_create refuses (a null pointer, 0 or more than 16 fields, a remote field, fields of
 * different dose grids, an objective on other dims or without terms, bad step bounds); n_plans of 0 or more than
 * RTD_PLANSET_MAX_PLANS; a variant with another kind or roi, a weight that is not positive and finite, a level that is not finite; an
 * objective with DVH or EUD terms; a plan or field index out of range; a blend coefficient that is negative or not finite.
 * RTD_ERR_NOT_READY: a field without a matrix. After a refusal every object is what it was.
 *
 * Measured (C3 on the 2 mm grid, 62.6 M entries, where a plain iteration takes 0.2845 ms): an iteration of the
 * set takes 0.3048 / 0.3525 / 0.3901 / 0.4933 / 0.8517 ms at 1 / 2 / 4 / 8 / 16 plans, which is 1.07 / 0.62 / 0.34 / 0.22 / 0.19 of
 * n_plans plain iterations. A set of ONE plan is slower than rtd_optimizer (by 7 %): use that for one plan. The gain per plan
 * flattens between 8 and 16 plans (0.062 and 0.053 ms per plan), where the gathers from the plan-minor volumes, not the matrix, are
 * what an iteration moves.
 *
 * Out of scope: DVH and EUD terms; a LET objective and an RBE model (there is no rtd_planset counterpart of
 * rtd_optimizer_set_let_objective / _set_rbe); robust and voxel-wise sets; nuclear_corr, remote fields and the rtd_plan_* path (as the
 * matrix itself).
 */
typedef struct rtd_planset_s* rtd_planset;
int rtd_planset_create(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_objective_term* variants,
                       uint32_t n_plans, const rtd_optimizer_options* o, rtd_planset* out);
int rtd_planset_set_weights(rtd_handle h, rtd_planset ps, uint32_t plan, uint32_t field_index, const float* dev_w);
int rtd_planset_run(rtd_handle h, rtd_planset ps, uint32_t n_iterations);
int rtd_planset_result(rtd_handle h, rtd_planset ps, uint32_t plan, rtd_optimizer_report* r, double* history, uint32_t capacity);
int rtd_planset_weights(rtd_handle h, rtd_planset ps, uint32_t plan, uint32_t field_index, int best, float* dev_w_out);
int rtd_planset_dose(rtd_handle h, rtd_planset ps, uint32_t plan, float* dev_dose_out);
int rtd_planset_values(rtd_handle h, rtd_planset ps, double* values_out);
int rtd_planset_blend(rtd_handle h, rtd_planset ps, const double* coeffs, uint32_t field_index, int best, float* dev_w_out);
int rtd_planset_destroy(rtd_handle h, rtd_planset ps);

/*
 * ---- L-BFGS with a line search on the device ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel or structure above changes). The spectral iteration
 * of rtd_optimizer_create has no line search and is not monotone. rtd_optimizer_create_lbfgs returns an ordinary rtd_optimizer whose
 * iteration is a projected limited-memory quasi-Newton step with a backtracking line search that needs no further matrix product:
 * between two feasible weight vectors the dose is linear, D (w + a (w_full - w)) = d0 + a (d1 - d0), so after ONE forward product for
 * the full step the objective at every trial step length is an evaluation of a mixed volume. rtd_optimizer_set_weights, _run, _result,
 * _weights, _dose and _destroy work on it; an iteration costs the two matrix products of the spectral one (one apply and one apply_t
 * per field).
 *
 * State on the device, owned by the optimiser: w, w_prev, grad, grad_prev, w_best, w_full (float32, n entries, the fields'
 * [L][ny][nx] maps concatenated in list order); a ring of m pairs s_i, y_i (each the float64 difference of float32 values, rounded
 * once to float32); the symmetric Gram matrix G (float64, (2m+1)^2) of the basis B = [s_0 .. s_{m-1}, y_0 .. y_{m-1}, ghat], a
 * pair's place in B being its ring slot; two dose volumes d0 (the tracked dose of w: rtd_optimizer_dose) and d1 and one g volume; a
 * record of scalars and the history.
 *
 * rtd_optimizer_run starts with d0 = sum_f Dij_f w_f when the dose is stale: after creation and after rtd_optimizer_set_weights (host
 * state known at launch time, not a device decision), by the spectral iteration's rule (step 1 of the block "Dose objectives and the
 * resident optimiser": the boxes of the fields 1.. cleared, field 0 with init = 1, the others accumulate). Then iteration k, launches
 * only, no decision on the host:
 *   1. rtd_objective_eval(d0) -> f_k, g; grad_f = Dij_f^T g per field; history[k] = f_k while k < history_capacity; if f_k < f_best:
 *      w_best = w, f_best = f_k, best_iteration = k (as the spectral iteration keeps them).
 *   2. Pair. If the previous iteration moved (a > 0): s = w - w_prev, y = grad - grad_prev. The pair enters the ring iff <s, y> > 0
 *      and <y, y> > 0 and both are finite; it takes the slot after the newest pair's (mod m), where the oldest pair leaves when the
 *      ring is full.
 *   3. Active set. ghat_j = (w_j == 0 && grad_j > 0) ? 0 : grad_j.
 *   4. One wide reduction: the products of s, y and ghat with every live vector of B, with ghat, s and y themselves: 3 (2m + 3)
 *      float64 sums (the pair's admission is decided from two of them, so the products with the pair it may replace are taken too),
 *      and max_j |P(w - grad)_j - w_j| in the cancellation-free form of the spectral iteration. Every sum by the optimiser's fixed
 *      tree: chunks of 2048 entries, one wave each, lane t adds the products of the entries t, t + 64, ... in order from +0.0
 *      (entries past n count as +0.0), butterfly (32, ..., 1); the chunk sums are added the same way. G takes the admitted pair's rows
 *      and columns and the row of ghat.
 *   5. The two-loop recursion on coefficients over B, every scalar in float64. q = ghat (coefficient 1 on ghat). For the pairs newest
 *      to oldest: alpha_i = <s_i, q> / <s_i, y_i>, then q -= alpha_i y_i. r = gamma q with gamma = <s, y> / <y, y> of the newest
 *      pair. For the pairs oldest to newest: beta = <y_i, r> / <s_i, y_i>, then r += (alpha_i - beta) s_i. An inner product <B_i, q>
 *      is the sum from 0.0 over the live indices j of B ascending of c_j * G[i][j], c the coefficients of q. The result is the
 *      coefficients delta of r (2m + 1 of them, 0 where a slot is not live). Without pairs delta is gamma0 on ghat alone, gamma0 =
 *      (initial_step > 0 ? initial_step : (mx > 0 ? 1 / mx : 0) with mx the max of step 4) times the stall factor of step 7.
 *   6. Direction and full step: dir_j = -(sum over the live i ascending, from 0.0, of delta_i * double(B_i[j])), 0 where j is active
 *      (w_j == 0 && grad_j > 0); w_full_j = float32(P(double(w_j) + dir_j)), P(x) = x > 0 ? x : +0. The same launch leaves the chunk
 *      sums of gp = <grad, w_full - w> = sum_j double(grad_j) * (double(w_full_j) - double(w_j)), by the tree of step 4. Then
 *      d1 = sum_f Dij_f w_full_f, the forward products by the rule above.
 *   7. Line search over K = 1 + max_halvings trial steps a_k = 2^-k. The trial dose of voxel v: t_0 = double(d1[v]), t_k = double(d0[v])
 *      + a_k * (double(d1[v]) - double(d0[v])) for k >= 1, no contraction. F_k is the objective of trial k: phi and every sum follow
 *      rtd_objective_eval's text exactly, so F_0 has the bits of rtd_objective_eval(d1). The first k with F_k <= f_k + (armijo_c1 *
 *      a_k) * gp is accepted (comparisons with a NaN are false: a trial that is not finite is never accepted). Then w_prev = w,
 *      grad_prev = grad and, k = 0: w = w_full and d0 = d1, copies of the bits; k >= 1: w_j = float32(double(w_j) + a_k *
 *      (double(w_full_j) - double(w_j))) and d0[v] = float32(t_k), over the bounding box of the fields' row boxes (outside the row
 *      boxes both volumes hold +0). After every unit step the tracked dose is the product's own bits; drift can accumulate only over
 *      consecutive backtracked steps.
 *      Not (gp < 0): a = 0 and nothing moves. With pairs held the ring is emptied and a reset is counted: the next iteration is a
 *      projected steepest-descent step. Without pairs the iterate is stationary for that step (gp = 0) and nothing is counted.
 *      No k accepted: a = 0, a stall is counted. With pairs held the ring is emptied; without pairs the stall factor (1 at the start)
 *      is multiplied by 2^-K. It returns to 1 at the next accepted step.
 *      f_k not finite: a = 0, nothing moves, counted in `guarded`; if no finite objective had been seen rtd_optimizer_result answers
 *      RTD_ERR_INVALID_ARG as it does for the spectral iteration. (w is NOT set back to w_best: no accepted step leads to such an f.)
 * Fixed summation trees and no float atomics: the same inputs give the same bits across calls, handles, processes and graph replays.
 *
 * rtd_optimizer_create_lbfgs  1 .. RTD_OPT_MAX_FIELDS local fields on the objective's dose grid, each with a matrix; options may be
 *                          NULL (rtd_default_lbfgs_options: memory 8, max_halvings 5, armijo_c1 1e-4, initial_step 0,
 *                          history_capacity 4096). Runs rtd_field_dose_influence_prepare where it has not run. Synchronous. It notes
 *                          every field's matrix and the objective: rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before its
 *                          first launch, once rtd_field_dose_influence has been called again on a field or an ROI or a term has been
 *                          added to the objective. Such an optimiser can only be destroyed.
 * rtd_optimizer_set_weights   as before; in addition the ring is emptied and the next run recomputes d0.
 * rtd_optimizer_result     f_last, f_best, best_iteration, iterations, history_len with their meaning above; step is the accepted a
 *                          of the last iteration (0: none); guarded counts the iterations whose objective was not finite.
 * rtd_optimizer_dose       d0: THE TRACKED DOSE OF THE CURRENT w, updated by the last iteration. This differs from the spectral
 *                          optimiser, whose volume holds the dose of the iterate that entered the last iteration.
 * rtd_optimizer_lbfgs_report  waits for the stream, like rtd_optimizer_result. RTD_ERR_INVALID_ARG on any other optimiser.
 * rtd_optimizer_lbfgs_buffers the optimiser's own device arrays, for inspection (read-only; they change with every iteration): no
 *                          synchronisation. delta: the 2m + 1 coefficients of step 5. gram: row-major (2m+1)^2. ring: [2m][n], the s
 *                          slots then the y slots. RTD_ERR_INVALID_ARG on any other optimiser.
 * RTD_ERR_INVALID_ARG: what rtd_optimizer_create refuses of a field list and an objective; an objective with DVH or EUD terms (D_v
 * and E couple the voxels of a structure, so the K-wide evaluation of step 7 does not apply); memory outside 1 .. 16, max_halvings
 * above 7, armijo_c1 outside (0, 0.5), an initial_step that is negative or not finite, a non-zero reserved word.
 * rtd_optimizer_set_let_objective, rtd_optimizer_set_rbe, rtd_optimizer_scenario_values and _scenario_dose refuse such an optimiser
 * with RTD_ERR_INVALID_ARG. RTD_ERR_NOT_READY: a field without a matrix.
 *
 * DVH and EUD terms in the line search and the compact matrix: rtd_optimizer_create_lbfgs_ex, the next block.
 * Out of scope: L-BFGS behind the robust, voxel-wise, plan-set, 4D, LET and RBE optimisers;
 * the Cauchy-point / subspace step of full L-BFGS-B; nuclear_corr and the rtd_plan_* path (as the matrix itself).
 */
enum { RTD_LBFGS_MAX_MEMORY = 16, RTD_LBFGS_MAX_HALVINGS = 7 };
typedef struct rtd_lbfgs_options {
    uint32_t memory;            /* m: pairs kept, 1 .. RTD_LBFGS_MAX_MEMORY */
    uint32_t max_halvings;      /* the line search tries K = 1 + max_halvings steps 2^-k; 0 .. RTD_LBFGS_MAX_HALVINGS */
    double armijo_c1;           /* sufficient decrease, in (0, 0.5) */
    double initial_step;        /* 0: the first rule of the spectral iteration, 1 / max_j |P(w - grad)_j - w_j|; else that scale */
    uint32_t history_capacity;  /* objective values kept on the device */
    int32_t reserved[5];        /* must be 0 */
} rtd_lbfgs_options;            /* 48 bytes */
typedef struct rtd_lbfgs_report {
    uint32_t pairs;             /* pairs held */
    uint32_t unit_steps;        /* iterations that accepted a = 1 */
    uint32_t backtracked_steps; /* iterations that accepted a < 1 */
    uint32_t halvings;          /* sum of k over the backtracked steps */
    uint32_t resets;            /* gp >= 0 with pairs held: the memory was dropped */
    uint32_t stalls;            /* no trial step accepted */
    int32_t last_trial;         /* k of the last iteration, -1: none accepted */
    int32_t pair_admitted;      /* the last iteration's pair entered the ring ... */
    int32_t pair_slot;          /* ... at this slot */
    int32_t ring_head;          /* the slot the next pair takes */
    double last_step;           /* the last accepted a (0: the last iteration accepted none) */
    double last_gp;             /* the last directional derivative <grad, w_full - w> */
    double stall_factor;        /* the factor on gamma0 */
    double trial_values[8];     /* F_k of the last line search, k < K */
    int32_t reserved[4];
} rtd_lbfgs_report;             /* 144 bytes */
typedef struct rtd_lbfgs_buffers {
    const float* w;
    const float* w_prev;
    const float* grad;
    const float* grad_prev;
    const float* w_full;
    const float* ring;
    const float* trial_dose;    /* d1 */
    const double* gram;
    const double* delta;
    uint32_t n, memory, n_chunks, n_trials;
} rtd_lbfgs_buffers;            /* 88 bytes */
void rtd_default_lbfgs_options(rtd_lbfgs_options* out);
int rtd_optimizer_create_lbfgs(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_lbfgs_options* o,
                               rtd_optimizer* out);
int rtd_optimizer_lbfgs_report(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_report* r);
int rtd_optimizer_lbfgs_buffers(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_buffers* b);

/*
 * ---- L-BFGS with DVH and EUD terms, and on the compact matrix ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point or structure above changes; rtd_optimizer_create_lbfgs keeps
 * its behaviour, its refusals and its bits). rtd_optimizer_create_lbfgs_ex returns an ordinary L-BFGS optimiser: rtd_optimizer_run,
 * _result, _weights, _set_weights, _dose, _lbfgs_report and _lbfgs_buffers work on it as on one of rtd_optimizer_create_lbfgs, and
 * rtd_optimizer_set_let_objective, _set_rbe, _scenario_values and _scenario_dose refuse it with the same codes. It accepts every term
 * kind of rtd_objective_eval, and with RTD_LBFGS_COMPACT its two products are rtd_field_dose_influence_apply_compact /
 * _apply_t_compact of the block below.
 *
 * THE LINE SEARCH WITH COUPLED TERMS. D_v (a DVH term) and E (an EUD term) couple all voxels of a structure, so every trial of step 7
 * needs a selection and a power sum of its own.
 *   If the objective has NO DVH or EUD term, the iteration is the one above, bit for bit: trials are evaluated on the float64 t_k, and
 *   rtd_optimizer_create_lbfgs_ex with flags 0 reproduces rtd_optimizer_create_lbfgs exactly.
 *   If it has one, every term of every trial is evaluated on the float32-rounded trial volume r_k[v] = float(t_k[v]), with t_0 =
 *   double(d1[v]) and t_k = double(d0[v]) + 2^-k * (double(d1[v]) - double(d0[v])), no contraction: exactly the expression step 7
 *   writes back as the new d0. (D_v is an order statistic of a float32 volume, selected on 32-bit keys, and the accepted trial
 *   becomes the tracked dose by that same rounding.) Two properties follow:
 *     1. F_k has the bits of rtd_objective_eval(r_k).values[0]: the same trees, the same selection, the same power sums. The DVH
 *        thresholds of trial k are rtd_objective_dose_at_volume(r_k), the E of an EUD term is rtd_objective_eud(r_k).
 *     2. After an accepted trial k the next iteration's f (its history entry) equals trial_values[k] bit for bit: no accepted step
 *        raises the objective, with no rounding allowance.
 *   Step 1 (value and gradient with D_v and K held fixed) is rtd_objective_eval as before. Per line search, whatever K is: three
 *   counting passes and one finish over (chunk, selection, trial) for the DVH terms, one sum and one finish for the EUD terms, the
 *   line kernel and the decision; launches only, no host read, integer counting and fixed float64 trees, so the iteration can be
 *   captured into a graph and gives the same bits across calls, handles, processes and replays.
 *
 * rtd_optimizer_create_lbfgs_ex  as rtd_optimizer_create_lbfgs, except that DVH and EUD terms are accepted.
 *                          flags: an unknown bit is RTD_ERR_INVALID_ARG.
 *                          Without RTD_LBFGS_COMPACT the refusals are those of rtd_optimizer_create_lbfgs,
 *                          RTD_ERR_NOT_READY for a field whose plain form has been released among them. With RTD_LBFGS_COMPACT every
 *                          field needs its compact form (RTD_ERR_NOT_READY otherwise, as rtd_optimizer_create_compact); creation
 *                          prepares nothing, so it works after release_plain; rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before
 *                          its first launch, once a field's matrix has been computed again. The per-trial arrays are allocated here
 *                          from the objective's own counts (at most 12.6 MB of histograms); RTD_ERR_OUT_OF_MEMORY keeps nothing.
 * rtd_optimizer_lbfgs_line_buffers  what the line search reads and leaves, for inspection (read-only; no synchronisation): d0, d1, and
 *                          of the last line search thresholds[k][t] = D_v of DVH term t at trial k and eud[k][t] = {E, K, value} of EUD
 *                          term t at trial k (entries of other terms are 0). Both are NULL when the objective has no DVH or EUD
 *                          term. RTD_ERR_INVALID_ARG on anything that is not an L-BFGS optimiser.
 *
 * Out of scope: L-BFGS behind the robust, voxel-wise, plan-set, 4D, LET and RBE optimisers; the Cauchy point of L-BFGS-B; any change
 * to the forward tree of the compact product.
 */
enum { RTD_LBFGS_COMPACT = 1u };   /* products read the fields' compact matrices */
typedef struct rtd_lbfgs_line_buffers {
    const float* d0;            /* the tracked dose of w */
    const float* d1;            /* the dose of w_full (rtd_lbfgs_buffers.trial_dose) */
    const float* thresholds;    /* float[n_trials][RTD_OBJ_MAX_TERMS], indexed by term; NULL without DVH or EUD terms */
    const double* eud;          /* double[n_trials][RTD_OBJ_MAX_TERMS][3]: E, K, value; NULL without DVH or EUD terms */
    uint32_t n_trials, n_terms;
    uint32_t reserved[6];
} rtd_lbfgs_line_buffers;       /* 64 bytes */
int rtd_optimizer_create_lbfgs_ex(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_lbfgs_options* o,
                                  uint32_t flags, rtd_optimizer* out);
int rtd_optimizer_lbfgs_line_buffers(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_line_buffers* b);

/*
 * ---- Hard dose constraints: an augmented Lagrangian resident on the device ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel or structure above changes). Everything above is a
 * penalty with a weight. A constraint is a bound that holds at the solution: "every voxel of the cord at most 45 Gy". The method is
 * the augmented Lagrangian around the resident spectral iteration: one multiplier per constrained voxel, a penalty rho that grows only
 * while the violation does not shrink, and no host round trip.
 *
 * CONSTRAINTS. rtd_objective_add_constraint adds one to an objective: it refers to a ROI of rtd_objective_add_roi (which may carry no
 * term), does not count towards RTD_OBJ_MAX_TERMS and lives in tables of its own. RTD_CON_MAX_DOSE: every voxel of the ROI at most
 * dose_level; RTD_CON_MIN_DOSE: every voxel at least dose_level; RTD_CON_MAX_MEAN / RTD_CON_MIN_MEAN: the same for the ROI's mean
 * dose. constraint_id (may be NULL) receives its number c, 0 .. RTD_CON_MAX_CONSTRAINTS - 1, in the order added.
 * rtd_objective_eval, _eval_voxelwise, _dvh, _dose_at_volume and _eud IGNORE constraints: they answer as before.
 * Every other creator (rtd_optimizer_create, _create_robust, _create_voxelwise, _create_4d, _create_lbfgs, _create_lbfgs_ex, the
 * _compact ones, rtd_planset_create) refuses an objective that has a constraint with RTD_ERR_INVALID_ARG before any launch, and so
 * does rtd_optimizer_set_let_objective for a LET objective that has one. An optimiser created BEFORE the constraint was added keeps
 * running on the terms alone (an L-BFGS one refuses its run, as after any change of its objective).
 *
 * DEVICE TABLES, built synchronously on first use: the union of the constrained ROIs ascending (union_voxels); per union voxel the
 * PER-VOXEL constraints (MAX_DOSE / MIN_DOSE) that hold it, in constraint order, as a CSR (entry_ptr[n_union + 1],
 * entry_constraint[n_entries]). A per-voxel multiplier is one float per CSR entry: lambda[n_entries]. The mean constraints have no CSR
 * entries: a union voxel carries a 16-bit mask of the mean constraints whose ROI holds it, and a mean constraint's multiplier is one
 * double, mu[c] of an array double[RTD_CON_MAX_CONSTRAINTS] indexed by the constraint's number (the entries of per-voxel constraints
 * are neither read nor written).
 *
 * THE ARITHMETIC. float64 throughout, no contraction, no atomics, sums by fixed trees. For constraint c on a ROI of N voxels with
 * level L: s = +1 for a MAX kind, -1 for a MIN kind; invN = 1.0 / N (host); rho the penalty.
 *   Per-voxel constraint, entry e at voxel v, lam = double(lambda[e]): h = s * (double(dose[v]) - L); u = lam + rho * h;
 *   a = u > 0 ? u : 0, and a = h where h is a NaN (the value is then not finite and the optimiser's guard acts as it does today).
 *     psi_c = (sum_e (a * a - lam * lam)) * (invN / (2 * rho)); the sum by rtd_objective_eval's tree over the union of the constrained
 *     ROIs (one thread per union voxel, blocks of 256, wave butterfly, (w0 + w1) + (w2 + w3), block b to lane b mod 64, butterfly).
 *     gc_e = s * (a * invN).
 *   Mean constraint: m = (sum_v double(dose[v])) * invN over the ROI, the sum by rtd_objective_eud's chunk tree (chunks of 2048,
 *   thread t adds the voxels t, t + 256, ... of its chunk in order, wave butterfly, (w0 + w1) + (w2 + w3); the chunk sums added the
 *   same way). h = s * (m - L); u = mu[c] + rho * h; a as above. psi_c = (a * a - mu[c] * mu[c]) / (2 * rho); gc = s * (a * invN) at
 *   every voxel of the ROI.
 *   Combined gradient: g[v] = float32(double(g_terms[v]) + G), G the sum from +0.0 of the gc of the voxel's constraints in constraint
 *   order (per-voxel and mean ones interleaved by number), g_terms[v] what rtd_objective_eval wrote (it writes every voxel of the
 *   union of ALL ROIs, 0 where a voxel has no term, so every constrained voxel has been written).
 *   Values: con_values[0] = the terms' values[0]; con_values[1 + c] = psi_c; values[0] = F = values[0] + psi_0 + psi_1 + ... in
 *   constraint order; values[1 + t] stay the terms'.
 *   Multiplier update with the same h: lambda[e] <- float32(min(max(u, 0), lambda_max)) where h is finite, otherwise lambda[e] stays;
 *   mu[c] likewise in float64. Per constraint from the same pass: max_violation = max(0, h) over the entries (a NaN h is left out;
 *   +inf counts), n_violating = the number of entries with h > tol (a mean constraint: 0 or 1).
 *
 * rtd_objective_eval_constrained   rtd_objective_eval followed by the launches above. dev_lambda float[n_entries], dev_mu
 *                          double[RTD_CON_MAX_CONSTRAINTS], dev_values double[1 + terms], dev_con_values double[1 + n_constraints],
 *                          dev_voxel_grad as rtd_objective_eval; all non-NULL. After the first call it only launches: no allocation,
 *                          copy or synchronisation, so it can be captured into a graph. An evaluation uses the objective's scratch.
 * rtd_objective_update_multipliers the update above, in place, and the violations to dev_out[n_constraints].
 * rtd_objective_constraint_violations  the same pass without the update.
 * rtd_objective_constraint_layout  the tables (device pointers owned by the objective, read-only, valid until the next ROI or
 *                          constraint is added) and their sizes.
 * RTD_ERR_INVALID_ARG: an objective without constraints (never silently forwarded) or, for eval_constrained, without terms; an unknown
 * kind or ROI; a dose level that is not finite; a non-zero reserved word; more than RTD_CON_MAX_CONSTRAINTS; rho that is not positive
 * and finite; lambda_max that is not positive; tol that is negative or a NaN.
 *
 * THE CONSTRAINED OPTIMISER. rtd_optimizer_create_constrained returns an ordinary rtd_optimizer on 1 .. RTD_OPT_MAX_FIELDS local
 * fields with plain matrices; the objective needs at least one term and one constraint. rtd_optimizer_run, _result, _weights,
 * _set_weights, _dose and _destroy work as on one of rtd_optimizer_create; rtd_optimizer_set_let_objective, _set_rbe, _scenario_values,
 * _scenario_dose and _lbfgs_* refuse it with RTD_ERR_INVALID_ARG. Multipliers start at 0, rho at rho0. Iteration k, counted over all
 * runs on the host (known at launch time; launches only, no decision on the host):
 *   0. If k > 0 and k % inner_iterations == 0, an OUTER UPDATE runs in front of the evaluation:
 *      (a) w = w_best if the current subproblem has a best iterate; (b) the forward product; (c) the means; (d) the multiplier update
 *      with the current rho and lambda_max, measured with tol = feasibility_tol; (e) v = the maximum over the constraints of
 *      max_violation. If this is not the first update and v > feasibility_tol and v > violation_shrink * v_prev then
 *      rho = min(rho * rho_growth, rho_max). v_prev = v. {k, rho, v} is appended to the outer history (while it has room). The record's
 *      f_best becomes +inf and its Barzilai-Borwein pair is dropped: the function has changed, and the best iterate and the pair of
 *      the old one mean nothing for it.
 *      On other iterations only the forward product runs.
 *   1. rtd_objective_eval_constrained with the optimiser's lambda, mu and rho: values[0] is F.
 *   2. The transposed product of the combined g.
 *   3. The steps 4 to 7 of the spectral iteration AS THEY ARE: history, best iterate and guard act on F.
 * The multiplier update is taken at the BEST iterate of each inner block, never at the current one: the spectral iteration is not
 * monotone, an excursion would land on the update and the penalty would grow without bound.
 * Consequences: w_best and f_best are those of the CURRENT subproblem. Run whole multiples of inner_iterations (the report carries
 * iterations_since_update). rtd_optimizer_result's "start unusable" answer can also mean a subproblem whose first value was not
 * finite. A captured run(n) replays the schedule it was captured with. An outer update costs one extra forward product.
 * It notes its matrices and its objective at creation: rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before its first launch,
 * once a field's matrix has been computed again or a ROI, term or constraint has been added.
 * rtd_optimizer_constraint_report  waits for the stream. f_objective is con_values[0] of the last evaluation; psi of the last
 *                          evaluation; max_violation and n_violating per constraint of the last outer update. outer_history
 *                          (may be NULL with capacity 0) receives min(capacity, outer_history_len) entries.
 * rtd_optimizer_constraint_buffers the optimiser's own device arrays, read-only, no synchronisation.
 * RTD_ERR_INVALID_ARG: what rtd_optimizer_create refuses; an objective without constraints; rho0 or rho_max not positive and finite or
 * rho_max < rho0; rho_growth < 1 or not finite; violation_shrink outside (0, 1]; feasibility_tol negative or not finite; lambda_max
 * not positive; inner_iterations 0; a non-zero reserved word.
 *
 * Out of scope: constraints behind L-BFGS (a monotone inner solver would suit the method better; it needs the constraint terms in the
 * K-wide line kernels and is the natural follow-up); the robust, voxel-wise, 4D, plan-set, LET, RBE and compact-matrix optimisers; DVH
 * and EUD constraints; upper bounds or minimum-MU rules on the weights; an on-device stopping rule; nuclear_corr, remote fields and
 * the rtd_plan_* path.
 */
enum { RTD_CON_MAX_DOSE = 0, RTD_CON_MIN_DOSE = 1, RTD_CON_MAX_MEAN = 2, RTD_CON_MIN_MEAN = 3 };
#define RTD_CON_MAX_CONSTRAINTS 16
typedef struct rtd_dose_constraint {
    int32_t kind;               /* RTD_CON_* */
    int32_t roi;                /* an id of rtd_objective_add_roi */
    double dose_level;
    int32_t reserved[4];        /* must be 0 */
} rtd_dose_constraint;          /* 32 bytes */
typedef struct rtd_constraint_layout {
    const int32_t* union_voxels;        /* [n_union], ascending */
    const int32_t* entry_ptr;           /* [n_union + 1] */
    const uint8_t* entry_constraint;    /* [n_entries] */
    uint32_t n_union, n_entries, n_constraints, n_mean;
    uint32_t reserved[4];
} rtd_constraint_layout;        /* 56 bytes */
typedef struct rtd_constraint_violation {
    double max_violation;
    uint32_t n_violating;
    uint32_t reserved;
} rtd_constraint_violation;     /* 16 bytes */
typedef struct rtd_constrained_options {
    double rho0, rho_growth, rho_max, violation_shrink, feasibility_tol, lambda_max;
    uint32_t inner_iterations, outer_capacity;
    int32_t reserved[4];        /* must be 0 */
} rtd_constrained_options;      /* 72 bytes */
typedef struct rtd_constraint_outer {
    uint64_t iteration;         /* k of the outer update */
    double rho;                 /* after the update's decision */
    double max_violation;       /* v */
} rtd_constraint_outer;         /* 24 bytes */
typedef struct rtd_constraint_report {
    double rho;
    double f_objective;         /* the terms alone, of the last evaluation */
    uint32_t outer_updates, rho_increases, iterations_since_update, n_constraints;
    uint32_t outer_history_len; /* min(outer_updates, outer_capacity) */
    uint32_t reserved[3];
    double psi[RTD_CON_MAX_CONSTRAINTS];
    double max_violation[RTD_CON_MAX_CONSTRAINTS];
    uint32_t n_violating[RTD_CON_MAX_CONSTRAINTS];
} rtd_constraint_report;        /* 368 bytes */
typedef struct rtd_constraint_buffers {
    const float* lambda;        /* [n_entries] */
    const double* mu;           /* [RTD_CON_MAX_CONSTRAINTS] */
    const double* rho;          /* one double */
    const double* con_values;   /* [1 + n_constraints] */
    const rtd_constraint_violation* violations;   /* [n_constraints], of the last outer update */
    const rtd_constraint_outer* outer_history;    /* [outer_capacity] */
    uint32_t n_entries, n_constraints, n_mean, outer_capacity;
} rtd_constraint_buffers;       /* 64 bytes */
int rtd_objective_add_constraint(rtd_handle h, rtd_objective obj, const rtd_dose_constraint* c, int32_t* constraint_id);
int rtd_objective_constraint_layout(rtd_handle h, rtd_objective obj, rtd_constraint_layout* layout);
int rtd_objective_eval_constrained(rtd_handle h, rtd_objective obj, const float* dev_dose, const float* dev_lambda, const double* dev_mu, double rho,
                                   double* dev_values, double* dev_con_values, float* dev_voxel_grad);
int rtd_objective_update_multipliers(rtd_handle h, rtd_objective obj, const float* dev_dose, double rho, double lambda_max, double tol, float* dev_lambda,
                                     double* dev_mu, rtd_constraint_violation* dev_out);
int rtd_objective_constraint_violations(rtd_handle h, rtd_objective obj, const float* dev_dose, double tol, rtd_constraint_violation* dev_out);
void rtd_default_constrained_options(rtd_constrained_options* out);
int rtd_optimizer_create_constrained(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o,
                                     const rtd_constrained_options* c, rtd_optimizer* out);
int rtd_optimizer_constraint_report(rtd_handle h, rtd_optimizer opt, rtd_constraint_report* r, rtd_constraint_outer* outer_history, uint32_t capacity);
int rtd_optimizer_constraint_buffers(rtd_handle h, rtd_optimizer opt, rtd_constraint_buffers* b);

/*
 * ---- Constrained L-BFGS: hard dose constraints behind the line search ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel or structure above changes).
 * The follow-up the block above names now exists: the augmented Lagrangian of that block around the L-BFGS iteration of "L-BFGS with
 * a line search on the device" instead of the spectral one. rtd_optimizer_create_constrained keeps its update at the best iterate. Here
 * the outer update is taken at the CURRENT iterate, because the inner solver is monotone: inside a block the L-BFGS iteration accepts
 * only trials with F_k <= f + c1 a gp and gp < 0, so the current iterate is the block's best. No weights are restored and no extra
 * forward product runs.
 *
 * rtd_optimizer_create_constrained_lbfgs returns an ordinary rtd_optimizer on 1 .. RTD_OPT_MAX_FIELDS local fields. flags is 0 or
 * RTD_LBFGS_COMPACT (the two products are then the compact ones, also after release_plain, as for rtd_optimizer_create_lbfgs_ex). The
 * objective needs at least one term, of any kind (DVH and EUD terms included), and at least one constraint. o and c may be NULL (the
 * defaults of rtd_default_lbfgs_options and rtd_default_constrained_options). It refuses what rtd_optimizer_create_lbfgs_ex and
 * rtd_optimizer_create_constrained refuse: the option ranges of both, a non-zero reserved word, an objective without terms or without
 * constraints, unknown bits in flags, remote fields (RTD_ERR_INVALID_ARG), a field without the matrix form asked for
 * (RTD_ERR_NOT_READY). A failed allocation (RTD_ERR_OUT_OF_MEMORY) keeps nothing and leaves every object usable.
 * rtd_optimizer_run, _result, _weights, _dose, _set_weights, _lbfgs_report, _lbfgs_buffers, _lbfgs_line_buffers, _constraint_report
 * (iterations_since_update by the same rule) and _constraint_buffers work on it as on their own kinds; _scenario_values,
 * _scenario_dose, _set_let_objective and _set_rbe refuse it, and so do plan sets. Every OTHER creator keeps refusing an objective that
 * has a constraint.
 *
 * THE ITERATION k, counted over all runs on the host (launches only, one chain, no decision on the host, so a run can be captured
 * into a graph; a captured run(n) replays the schedule it was captured with). F = f + sum_c psi_c is the function
 * rtd_objective_eval_constrained evaluates with the optimiser's lambda, mu and rho.
 *   0. If k > 0 and k % inner_iterations == 0, an OUTER UPDATE runs on the tracked dose of the current w (after the forward product
 *      of a stale tracked dose, as in the L-BFGS iteration): the means, the multiplier update with the current rho and lambda_max,
 *      measured with tol = feasibility_tol, and the decision (e) of the block above with its penalty rule and its outer history.
 *      f_best becomes +inf, so the evaluation that follows makes the current w the new subproblem's best iterate. Then the L-BFGS
 *      memory is dropped as after rtd_optimizer_set_weights (a pair w - w_prev, grad - grad_prev would mix two functions, and the ring
 *      describes the old one): ring head, stall factor and counters stay.
 *   1. rtd_objective_eval_constrained on the tracked dose: values[0] = F, the voxel gradient carries the constraints' share; then the
 *      transposed products, plain or compact.
 *   2. Steps 2 to 6 of the L-BFGS iteration unchanged, on F and its gradient.
 *   3. THE LINE SEARCH. Every trial k < K = 1 + max_halvings is evaluated on the float32 volume
 *      r_k[v] = k == 0 ? d1[v] : float32(double(d0[v]) + 2^-k * (double(d1[v]) - double(d0[v]))), whether or not the objective has DVH
 *      or EUD terms: the terms as in "L-BFGS with DVH and EUD terms", the constraints with the arithmetic and the trees of the block
 *      above (psi_{c,k} of a per-voxel constraint by rtd_objective_eval's tree over the union of the constrained ROIs, the mean
 *      m_{c,k} by the chunk tree). F_k = the terms from +0.0 in term order, then + psi_{0,k} + psi_{1,k} + ... in constraint order:
 *      F_k has the bits of values[0] of rtd_objective_eval_constrained(r_k). Then the decision of the L-BFGS iteration unchanged.
 *      Inside a block the next history entry equals the accepted F_k bit for bit. Across an outer update F changes and it does not.
 *   4. The weight and dose updates of the L-BFGS iteration unchanged.
 * w_best and f_best are those of the current subproblem; with a monotone inner solver that is the current iterate after every
 * accepted step. It notes its matrices and its objective at creation: rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before its
 * first launch, once a field's matrix has been computed again or a ROI, term or constraint has been added.
 *
 * rtd_optimizer_lbfgs_constraint_line  the device arrays the last line search left, read-only, no synchronisation:
 *                          con_trial[k][0] = the terms' value at trial k, con_trial[k][1 + c] = psi_{c,k} (rows of
 *                          1 + RTD_CON_MAX_CONSTRAINTS doubles), mean_trial[k][c] = m_{c,k} of a mean constraint (rows of
 *                          RTD_CON_MAX_CONSTRAINTS doubles; +0 for a per-voxel constraint). RTD_ERR_INVALID_ARG on any other optimiser.
 * rtd_objective_constraint_trials      the constraint half of the line search as a call of its own, on two float32 volumes and with
 *                          the workspace of the objective (the optimiser calls the same internal function): dev_psi[k][c] = psi_{c,k}
 *                          and dev_mean[k][c] = m_{c,k}, rows of RTD_CON_MAX_CONSTRAINTS doubles, for k < n_trials; entries past the
 *                          objective's constraints, and dev_mean of a per-voxel constraint, are +0. dev_lambda and dev_mu as for
 *                          rtd_objective_eval_constrained. After the first call it only launches. RTD_ERR_INVALID_ARG: n_trials
 *                          outside 1 .. 8, rho not positive and finite, a NULL pointer, an objective without constraints.
 *
 * Out of scope: the robust, voxel-wise, 4D, plan-set, LET and RBE optimisers; DVH and EUD constraints;
 * bounds or minimum-MU rules on the weights; an on-device stopping rule.
 */
typedef struct rtd_lbfgs_constraint_line_buffers {
    const double* con_trial;    /* double[n_trials][1 + RTD_CON_MAX_CONSTRAINTS]: the terms' value, then psi_c */
    const double* mean_trial;   /* double[n_trials][RTD_CON_MAX_CONSTRAINTS]: m_c of the mean constraints */
    uint32_t n_trials, n_constraints;
    uint32_t reserved[4];
} rtd_lbfgs_constraint_line_buffers;   /* 40 bytes */
int rtd_optimizer_create_constrained_lbfgs(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_lbfgs_options* o,
                                           const rtd_constrained_options* c, uint32_t flags, rtd_optimizer* out);
int rtd_optimizer_lbfgs_constraint_line(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_constraint_line_buffers* b);
int rtd_objective_constraint_trials(rtd_handle h, rtd_objective obj, const float* dev_d0, const float* dev_d1, uint32_t n_trials, const float* dev_lambda,
                                    const double* dev_mu, double rho, double* dev_psi, double* dev_mean);

/*
 * ---- Compact dose-influence matrix: fp16 values, 16-bit indices, products of its own ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point, kernel or structure above changes). The plain form of a
 * field's matrix keeps 16 bytes per entry: 4 B row + 4 B value in the CSC, 4 B column + 4 B value in the row-major companion. The two
 * products are bound by those bytes. The compact form is opt-in and keeps 4 B per entry on each side where the shapes allow.
 *
 * VALUES. The two sides share one scale s_j (float32) per column j (spot):
 *   m_j is the largest |v| of column j; e_j is the exponent of frexp(m_j), so m_j = f 2^e_j with f in [0.5, 1); s_j = 2^(e_j - 15).
 *   The code of an entry is half_rne(v * 2^(15 - e_j)): an IEEE binary16, round to nearest even. The product by a power of two is
 *   exact. A column that is empty or all zero gets s_j = 1 and zero codes.
 * The dequantised value is v^ = float(code) * s_j, exact in float32, and |v^ - v| <= max(2^-11 |v|, 2^-25 s_j).
 * The build is refused with RTD_ERR_INVALID_ARG, and leaves the field as it was, if a value is not finite or a column has
 * 0 < m_j < 2^-100 (decided on the device, read once by the synchronous build), or if the field has more than 65 536 spots.
 *
 * COMPANION SIDE (forward product). Per entry a binary16 code and a uint16 column, rows in the plain companion's order (the voxels
 * of the row box, x fastest), columns ascending. The forward tree has G lanes per row (lanes_per_row, 16 or 32), each taking E
 * consecutive entries per trip (entries_per_lane, 1, 2 or 4). With E == 1 the row pointers are the plain companion's. With E > 1
 * every row is padded to a multiple of E (pads at its end: code +0, column 0) and the side has row pointers of its own: row r's
 * entries start at row_ptr[r] & ~(E - 1), its pads number row_ptr[r] & (E - 1), row_ptr[n_rows] is the number of entries, pads included.
 *
 * CSC SIDE (transposed product). Per entry a binary16 code and a uint16 offset; per group of 64 consecutive entries of a column one
 * int32 base, the voxel of the group's first entry. Groups restart at every chunk of 2048 entries of a column (the chunks of
 * rtd_field_dose_influence_apply_t): group g of the field's chunk c is csc_base[32 c + g] (0 where a short chunk has no such group).
 * Rows ascend within a column: voxel = base + offset. If any group of the field spans more than 65 535 voxels (a dose-grid slice
 * nx * ny that large), the side keeps the plain 32-bit rows instead of the offsets: row_bits = 32, 6 B per entry.
 *
 * THE PRODUCTS. Every product is rounded to float32 before it is added, every sum starts from +0, no float atomics: the same inputs
 * give the same bits across calls, handles, processes and graph replays.
 *   rtd_field_dose_influence_apply_compact    ws[j] = fl(w[j] * s_j); then per voxel of the row box lane t of G adds the products
 *                                             fl(float(code) * ws[col]) of the row's entries (k G + t) E + e, e = 0 .. E - 1, then
 *                                             k = 0, 1, ..., in that order; the G lane sums in a butterfly at distances G / 2 .. 1. A pad
 *                                             is never multiplied. init, the row box and an empty matrix as rtd_field_dose_influence_apply.
 *   rtd_field_dose_influence_apply_t_compact  the chunks and both trees of rtd_field_dose_influence_apply_t on the products
 *                                             fl(float(code) * g[voxel]); dev_spot_grad[j] = fl(s_j * sum). Empty columns give +0.
 * Both are launches only on the handle's stream, allocate nothing and can be captured into a graph.
 *
 * rtd_field_dose_influence_compact      synchronous. Runs rtd_field_dose_influence_prepare where it has not run, builds the scales and
 *                          both sides. options may be NULL. With release_plain = 1 it then frees the CSC's rows (unless row_bits = 32)
 *                          and values, the plain companion's columns and values and any LET values. From there until the next
 *                          rtd_field_dose_influence every consumer of the plain form answers RTD_ERR_NOT_READY with a message that
 *                          names release_plain: rtd_field_dose_influence_copy, _device, _apply, _apply_t, _apply_set, _apply_t_set,
 *                          rtd_field_let_*, every optimiser and plan-set creator but rtd_optimizer_create_compact, and the run of an
 *                          optimiser or plan set created before. The next rtd_field_dose_influence frees the compact form with the
 *                          matrix it belonged to. A second call keeps the form that stands (and releases, if asked).
 *                          RTD_ERR_NOT_READY: no matrix. RTD_ERR_INVALID_ARG: a remote or nuclear_corr field, a non-zero reserved
 *                          word, release_plain above 1, the refusals of the format above.
 *                          Environment (read by the build; for the profiles): RTD_DIJC_LANES (16 or 32) and RTD_DIJC_PER (1, 2 or 4)
 *                          choose the forward tree; the default is 16 lanes, 4 entries.
 * rtd_field_dose_influence_compact_info     what was built, the bytes it keeps, and the bytes the plain form's bulk keeps or kept.
 * rtd_field_dose_influence_compact_device   the device pointers (owned by the field), for inspection.
 * rtd_optimizer_create_compact  rtd_optimizer_create's spectral optimiser, every term kind, with the two compact products in place of
 *                          the plain ones. Every field needs a compact form (RTD_ERR_NOT_READY). It notes every field's matrix:
 *                          rtd_optimizer_run refuses with RTD_ERR_NOT_READY, before its first launch, once rtd_field_dose_influence
 *                          has been called again on a field. rtd_optimizer_set_let_objective and rtd_optimizer_set_rbe refuse it
 *                          with RTD_ERR_INVALID_ARG.
 *
 * Out of scope: L-BFGS, robust, voxel-wise, plan-set and 4D optimisers on the compact form; compact LET values; plan-minor products
 * with several right-hand sides; nuclear_corr and the rtd_plan_* path (as the matrix itself).
 */
typedef struct rtd_dij_compact_options {
    uint32_t release_plain;     /* 1: free the plain form's bulk once the compact form stands */
    int32_t reserved[7];        /* must be 0 */
} rtd_dij_compact_options;      /* 32 bytes */
typedef struct rtd_dij_compact_info {
    uint32_t value_bits;        /* 16 */
    uint32_t col_bits;          /* 16 */
    uint32_t row_bits;          /* 16: offsets from group bases; 32: the plain rows */
    uint32_t lanes_per_row;     /* G */
    uint32_t entries_per_lane;  /* E */
    uint32_t plain_released;
    uint64_t nnz;
    uint64_t row_entries;       /* entries of the companion side, pads included */
    uint64_t compact_bytes;     /* kept by the compact form's own buffers */
    uint64_t plain_bytes;       /* the plain form's bulk (CSC rows and values, companion columns and values, LET values): kept, or as
                                   it was when it was released */
    uint64_t released_bytes;    /* of those, freed by release_plain (0: not released) */
    int32_t reserved[4];
} rtd_dij_compact_info;         /* 80 bytes */
typedef struct rtd_dij_compact_device {
    const float* scale;         /* [n_spots] */
    const int64_t* col_ptr;     /* [n_spots + 1], the plain CSC's */
    const uint16_t* csc_code;   /* [nnz] */
    const uint16_t* csc_offset; /* [nnz]; NULL when row_bits = 32 */
    const int32_t* csc_base;    /* [n_groups] */
    const int32_t* csc_rows;    /* [nnz] when row_bits = 32, else NULL */
    const int64_t* row_ptr;     /* [n_rows + 1] */
    const uint16_t* row_code;   /* [row_entries] */
    const uint16_t* row_col;    /* [row_entries] */
    uint64_t nnz, n_groups, n_rows, row_entries;
    int32_t box[6];             /* the row box: x0, y0, z0, width, height, depth */
} rtd_dij_compact_device;       /* 128 bytes */
void rtd_default_dij_compact_options(rtd_dij_compact_options* out);
int rtd_field_dose_influence_compact(rtd_handle h, rtd_field f, const rtd_dij_compact_options* o);
int rtd_field_dose_influence_compact_info(rtd_handle h, rtd_field f, rtd_dij_compact_info* info);
int rtd_field_dose_influence_compact_device(rtd_handle h, rtd_field f, rtd_dij_compact_device* d);
int rtd_field_dose_influence_apply_compact(rtd_handle h, rtd_field f, const float* dev_spot_weights, float* dev_dose, int init);
int rtd_field_dose_influence_apply_t_compact(rtd_handle h, rtd_field f, const float* dev_voxel_weights, float* dev_spot_grad);
int rtd_optimizer_create_compact(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o,
                                 rtd_optimizer* out);

/*
 * ---- Robust and voxel-wise optimisation on the compact matrix ----
 *
 * Additive to the blocks above (RTD_ABI_VERSION stays 3; no entry point or structure above changes what it answers). A robust plan
 * holds S x F matrices and reads each of them in every iteration, so it is where the bytes of the compact form count most; with
 * release_plain it is also the only way such a plan fits the card once the plain forms would not. The two creators below lift the
 * restriction of the block above for the scenario-wise robust optimiser and the voxel-wise worst case.
 *
 * rtd_optimizer_create_robust_compact     rtd_optimizer_create_robust (same arguments, same checks, every term kind it accepts) on
 *                          the compact forms of the S x F fields. The iteration is that optimiser's; only its two products change:
 *                          step 1 is rtd_field_dose_influence_apply_compact(init = 0) per field into a zeroed volume, step 4 is
 *                          rtd_field_dose_influence_apply_t_compact, bit for bit. Per field position one launch covers every scenario
 *                          (the single-matrix kernels' bodies with the scenario as the grid's y; the scaled weights
 *                          ws_s[j] = fl(w[j] * s_{s,j}) go into each field's own workspace; scenarios with lambda_s = 0 do no
 *                          transposed work). RTD_ROBUST_NO_BATCH (read at creation) issues the single-matrix compact products
 *                          scenario by scenario instead: the same bits.
 *                          The width of the CSC side's rows (row_bits) may differ between the scenarios of one position. The forward
 *                          tree may not: field f of every scenario must have the lanes_per_row and entries_per_lane of field f of
 *                          scenario 0 (RTD_ERR_INVALID_ARG).
 *                          Every field needs a compact form (RTD_ERR_NOT_READY); no rtd_field_dose_influence_prepare runs, so creation
 *                          works after release_plain. It notes every field's matrix: rtd_optimizer_run refuses with
 *                          RTD_ERR_NOT_READY, before its first launch, once rtd_field_dose_influence has been called again on any of
 *                          the S x F fields.
 * rtd_optimizer_create_voxelwise_compact  rtd_optimizer_create_voxelwise likewise (it refuses DVH and EUD terms as that one does).
 * Both return an ordinary rtd_optimizer: rtd_optimizer_set_weights, _run, _result, _weights, _dose, _scenario_values, _scenario_dose
 * and _destroy work as on their plain siblings; rtd_optimizer_set_let_objective and rtd_optimizer_set_rbe refuse them with
 * RTD_ERR_INVALID_ARG. rtd_optimizer_create_robust and rtd_optimizer_create_voxelwise themselves still answer RTD_ERR_NOT_READY on
 * a field whose plain form has been released.
 * Environment (read by rtd_field_dose_influence_compact; for tests and profiles): RTD_DIJC_ROWS32=1 makes the build keep the 32-bit
 * rows whatever the spans are, so that one plan can mix the two widths.
 *
 * Out of scope: L-BFGS, plan-set and 4D optimisers on the compact form; compact LET values; RBE and LET objectives in robust optimisers.
 */
int rtd_optimizer_create_robust_compact(rtd_handle h, const rtd_field* fields /* [S][F] scenario-major */, uint32_t n_fields,
                                        const rtd_robust_options* robust, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);
int rtd_optimizer_create_voxelwise_compact(rtd_handle h, const rtd_field* fields, uint32_t n_fields, uint32_t n_scenarios,
                                           rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);

/*
 * ---- Multi-GPU plans behind the boundary (SURVEY.md 8(b) "Threading": one handle and one host thread per device) ----
 *
 * rtd_plan is the reference-shaped call on several GPUs of one process: the 4-beam cudaWrapperProtons of the C++ shim uses
 * 4 GPUs. Beams are dealt round-robin to the devices; every device computes the BEV dose of its beams, the packed BEV
 * slabs (~10 MB each) are pulled by the other devices over xGMI (peer copies), and every device transfers ALL beams, in
 * beam order, into its own z-slab of the dose volume — uploaded from and downloaded to the caller's host buffer by that
 * device alone, so the PCIe legs (the bulk of the reference's "total global execution time", kernel_wrapper.cu:410-414,
 * 1356-1360) run in parallel as well. No dose data crosses between GPUs, and every voxel sees the same `+=` order as on one
 * GPU: the result equals rtd_compute bit for bit.
 * device_ids may repeat an id (several handles on one GPU) — used by the tests on one-GPU machines.
 * Environment: RTD_PLAN_TRANSPORT=rccl moves the slabs with ncclBroadcast (communicators from ncclCommInitAll, librccl opened on
 * demand; distinct device ids required) instead of peer copies.
 */
typedef struct rtd_plan_s* rtd_plan_t;

typedef struct rtd_plan_timing {
    float total_ms;        /* wall clock of rtd_plan_compute: dose up, all beams, dose down ("Total global execution time
                              (excluding GPU initialisation)", kernel_wrapper.cu:1356-1360)                              */
    float upload_ms;       /* slowest device: slab allocation + issuing the upload of the dose block the plan can change (the
                              copy itself runs beside the kernels; the transfers wait for it)                                */
    float bev_ms;          /* slowest device: its beams up to the BEV dose, slabs exported                               */
    float exchange_ms;     /* slowest device: pulling the other devices' slabs                                          */
    float transfer_ms;     /* slowest device: transfers of all beams into its slab (includes waiting for the upload)    */
    float download_ms;     /* slowest device: the changed block of its slab, device -> host                             */
    int32_t n_devices;
    int32_t reserved[3];
} rtd_plan_timing;

int rtd_plan_create(const int* device_ids, int n_devices, rtd_plan_t* out);
int rtd_plan_destroy(rtd_plan_t p);
const char* rtd_plan_last_error(rtd_plan_t p);
int rtd_plan_set_options(rtd_plan_t p, const rtd_options* opt);
int rtd_plan_set_luts(rtd_plan_t p, const rtd_luts* luts);                          /* replicated on every device */
int rtd_plan_load_luts_dir(rtd_plan_t p, const char* dir, int water_cube_test);
int rtd_plan_set_ct(rtd_plan_t p, const float* hu_plus_1000, const uint32_t dims[3]);            /* replicated, uploads in parallel */
int rtd_plan_set_ct_deferred(rtd_plan_t p, const float* hu_plus_1000, const uint32_t dims[3]);   /* rtd_set_ct_deferred on every device */
/* per_beam_timing: NULL or n_beams records (filled by the device that computed the beam). */
int rtd_plan_compute(rtd_plan_t p, const rtd_beam* beams, int n_beams, float* dose_inout, const uint32_t dose_dims[3],
                     rtd_timing* per_beam_timing, rtd_plan_timing* plan_timing);

#ifdef __cplusplus
}
#endif

#endif /* RTD_H */
