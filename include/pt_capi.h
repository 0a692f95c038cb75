/*
 * pt_capi.h — C-ABI of the MI355X path-tracing library (libpt_hip.so).
 *
 * Drop-in boundary for the reference's per-pixel radiance loop
 * (/root/reference/main.py:186-271).  The reference has no native FFI: its
 * only operator seam is two Python callables handed to
 * multiprocessing.Pool.apply_async —
 *     intersect_objects(ray, objects, light_obj)      main.py:83, :200-201
 *     compute_color(scene, obj, point, normal)        main.py:142, :218-219
 * — driven by the spp x bounce loop of main.py:186-271.  This header replaces
 * that whole loop (pt_render*), and exposes the two callables as batched
 * entry points (pt_intersect_objects, pt_compute_color) so a caller can swap
 * them in one at a time.  Python binds it with ctypes
 * (pathtracerpython_amd/_native.py); INTEGRATION.md shows the binding.
 *
 * Conventions: plain C types only.  Return 0 on success, a negative
 * PT_E* code on failure; pt_last_error() gives a thread-local message.  Input
 * arrays are caller-owned and read-only; the library copies what it needs to
 * device memory at pt_scene_create.  Output buffers are caller-allocated.
 * A pt_scene handle is not re-entrant (one call at a time per handle); the
 * library orders the launches made on one handle (each waits on the GPU for
 * the previous one, whatever stream either was issued on), because they share
 * the handle's device scratch.
 */
#ifndef PT_CAPI_H
#define PT_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API_VERSION 7

/* error codes */
#define PT_OK 0
#define PT_EINVAL (-1)     /* bad argument (shape, range, null pointer) */
#define PT_EHIP (-2)       /* HIP runtime error */
#define PT_ENOMEM (-3)     /* device or host allocation failed */
#define PT_ENODEV (-4)     /* no usable gfx950 device */
#define PT_EUNSUPPORTED (-5) /* pt_obj_load: input outside the fast reader's subset */
#define PT_ETIMEOUT (-6)   /* pt_wait_flags: the flags did not arrive in time */

/* pt_render flags */
#define PT_FLAG_RR (1u << 0)           /* Russian roulette (build extension) */
#define PT_FLAG_FORCE_F64 (1u << 1)    /* send every intersection test to the
                                          f64 evaluator (self-check mode) */
#define PT_FLAG_COUNT (1u << 2)        /* fill pt_stats counters (slower) */
#define PT_FLAG_OUT_F64 (1u << 3)      /* framebuffer elements are float64
                                          (default float32)              */
#define PT_FLAG_MEGAKERNEL (1u << 4)   /* scenes with a BVH: render with the
                                          single kernel instead of the
                                          wavefront kernels (same result) */
#define PT_FLAG_WALK_COUNT (1u << 5)   /* wavefront renders (BVH scenes): count
                                          the walks' queries, node visits and
                                          leaf-unit tests into pt_stats
                                          (counting kernels; synchronous)  */
#define PT_FLAG_KERNEL_TIMES (1u << 6) /* wavefront renders: per-kernel HIP-event
                                          times into pt_stats (synchronous; the
                                          two walks of a step run one after the
                                          other, so each time is its own)   */
/* bit 7: reserved (v4's PT_FLAG_TREE_WALK, retired in v5 with the grid-walk
   experiment it selected against; the library rejects it)                */
#define PT_FLAG_RESERVED7 (1u << 7)
/* Antialiasing (build extension; v7, additive): sample s of
 * pixel k = ix*H + iy uses its own primary ray.  s is the absolute sample
 * index: sample_begin + ... in a uniform render, n[e] + ... in an accumulator
 * pass.
 *  1. Jitter block: (w0, w1, ., .) = Philox4x32-10(key = seed,
 *     ctr = (k, s, 0xFFFFFFFF, 0)).  Bounce 0xFFFFFFFF is used by no path
 *     (bounces are non-negative int32).
 *  2. Offsets: jx = u_of(w0) - 0.5, jy = u_of(w1) - 0.5, both in [-0.5, 0.5)
 *     and exact in f64 (u_of(w) = (w >> 8) / 2^24).  The filter is a box one
 *     pixel spacing wide.
 *  3. Pixel spacing: dx = W > 1 ? (x1 - x0)/(W - 1) : 0, dy the same with H
 *     and the y bounds (ortho = x0 y0 x1 y1).
 *  4. Shifted window: ax = jx*dx; x0' = x0 + ax; x1' = x1 + ax; the same for
 *     y.  Every operation is rounded on its own.
 *  5. Primary ray: x = linspace_at(x0', x1', W, ix), y = linspace_at(y0', y1',
 *     H, iy) (np.linspace), d0 = (x - eye.x, y - eye.y, 0 - eye.z), origin
 *     eye; its closest hit is found as for any primary ray.
 *  6. The rest of sample s is unchanged: the same counters (k, s, bounce,
 *     slot>>2) and bounce loop.  A primary ray that escapes contributes 0,
 *     one that hits the light contributes light_rgb — per sample, not per
 *     pixel.  bounces <= 0 gives 0.
 * So sample s of pixel k is the reference's sample s of pixel k on a scene
 * whose ortho is (x0', y0', x1', y1'), and it depends on (seed, k, s) only:
 * the same draw in whichever launch, pass, band or resumed run takes it.
 * Allowed beside it: PT_FLAG_RR, PT_FLAG_FORCE_F64, PT_FLAG_OUT_F64,
 * PT_FLAG_MEGAKERNEL; with PT_FLAG_COUNT it is PT_EINVAL.  Scenes with a BVH
 * render through the wavefront kernels under the conditions of a launch
 * without the flag (each path slot starts a closest query from the eye per
 * sample; the same lanes per pixel, so the frame and S, Q, n are the single
 * kernel's bit for bit).  PT_FLAG_WALK_COUNT and PT_FLAG_KERNEL_TIMES are
 * accepted where the launch takes the wavefront kernels and fill pt_stats as
 * for a launch without the flag; where it takes the single kernel (no BVH,
 * PT_FLAG_MEGAKERNEL, PT_FLAG_FORCE_F64, a tree deeper than the walk stack,
 * 2^29 path slots or more) they are PT_EINVAL.  An accumulator remembers the bit of its
 * first pass since pt_accum_reset / pt_accum_create / pt_accum_write / an
 * imported tile and refuses a pass with the other value (PT_EINVAL): mixed
 * passes would mix two definitions of sample s.  Features and the denoiser
 * keep the centre ray.                                                    */
#define PT_FLAG_AA (1u << 8)
/* Thin-lens camera (build extension; v7, additive): depth of
 * field, a lens point per sample.  The scene is created with a lens
 * (pt_scene_create_lens): a radius R >= 0 and the z of the focal plane zf.
 * ez = eye[2]; the screen is the plane z = 0.  Sample s (absolute, as for
 * PT_FLAG_AA) of pixel k = ix*H + iy:
 *  1. Block: (w0, w1, w2, w3) = Philox4x32-10(key = seed,
 *     ctr = (k, s, 0xFFFFFFFF, 0)) — PT_FLAG_AA's jitter block; words 2 and 3
 *     are the lens's.
 *  2. Jitter: with PT_FLAG_AA (jx, jy) as in its rule; without it jx = jy = 0.
 *  3. Lens point: r = R * sqrt_d(u_of(w2)); phi = 6.283185307179586 * u_of(w3);
 *     (sn, cs) = sincos_small(phi); lx = r*cs; ly = r*sn;
 *     ex' = eye.x + lx; ey' = eye.y + ly; ez' = ez.  (sqrt_d, sincos_small:
 *     csrc/pt_math.h — within 3 ulp and 2^-52 absolute of the exact values.)
 *  4. Window: kappa = (0 - zf)/(ez - zf) (the lens offset scaled from the
 *     lens plane to z = 0, the focal plane being the fixed point);
 *     bx = jx*dx + lx*kappa; by = jy*dy + ly*kappa (dx, dy: PT_FLAG_AA's pixel
 *     spacing); x0' = x0 + bx; x1' = x1 + bx; the same for y.
 *  5. Primary ray: x = linspace_at(x0', x1', W, ix), y likewise,
 *     d0 = (x - ex', y - ey', 0 - ez), origin eye'.
 *  6. The rest of sample s is unchanged, except that eye' stands wherever the
 *     sample reads the eye (the specular term of the bounce included).  An
 *     escape contributes 0, a light hit light_rgb, per sample; bounces <= 0
 *     gives 0.
 * Every f64 operation is rounded on its own.  So sample s of pixel k is the
 * reference's sample on a descriptor with eye = eye' and ortho = (x0', y0',
 * x1', y1'); it depends on (seed, k, s, R, zf) only.  R = 0 is the pinhole
 * (with PT_FLAG_AA: the antialiased render, bit for bit); zf = 0 moves only the
 * eye.  The aperture is a uniform disc by the polar map.
 * The flag on a scene without a lens is PT_EINVAL; a lens scene rendered
 * without the flag is the pinhole render.  Allowed beside it: PT_FLAG_AA,
 * PT_FLAG_RR, PT_FLAG_FORCE_F64, PT_FLAG_OUT_F64, PT_FLAG_MEGAKERNEL; with
 * PT_FLAG_COUNT, PT_FLAG_WALK_COUNT or PT_FLAG_KERNEL_TIMES it is PT_EINVAL.
 * Scenes with a BVH render through the wavefront kernels under the conditions
 * of a launch without the flag (each path slot starts a closest query from its
 * sample's lens point, with or without PT_FLAG_AA; the same lanes per pixel,
 * so the frame and S, Q, n are the single kernel's bit for bit); the single
 * kernel takes the launch on a scene without a BVH, with PT_FLAG_MEGAKERNEL or
 * PT_FLAG_FORCE_F64, on a tree deeper than the walk stack and at 2^29 path
 * slots or more (pt_last_launch_info tells which).  An accumulator remembers
 * the bit as it remembers PT_FLAG_AA and refuses a mixed pass.  Features and
 * the denoiser keep the centre ray from the eye.                           */
#define PT_FLAG_LENS (1u << 9)
/* pt_radiance / pt_radiance_device only (v7, additive): the launch takes the
 * single kernel k_render_rays whatever the scene (see the routing paragraph
 * under pt_radiance; what PT_FLAG_MEGAKERNEL is to a frame — that flag stays
 * refused there).  Every other entry answers PT_EINVAL.                      */
#define PT_FLAG_RAYS_SINGLE (1u << 10)

/*
 * Flattened scene, as produced by scene_reader.Scene
 * (/root/reference/scene_reader.py:107-188).  Triangles are ordered exactly
 * as the reference iterates them in intersect_objects (main.py:91-96):
 * every object's triangles in scene order, then the light's triangles.
 */
typedef struct pt_scene_desc {
    int32_t n_tri;           /* all triangles (objects + light)               */
    int32_t n_obj_tri;       /* leading triangles that belong to objects      */
    int32_t n_obj;           /* objects (materials); light has index n_obj    */
    int32_t reserved;
    const double* tri_v;     /* [n_tri][3][3] vertices v1,v2,v3 as read       */
    const double* tri_n;     /* [n_tri][3] Obj.normals (scene_reader.py:5-8)  */
    const double* tri_area;  /* [n_tri]    Obj.areas  (vector.py:164-165)     */
    const int32_t* tri_obj;  /* [n_tri] object index; light triangles: n_obj  */
    const double* mat;       /* [n_obj][8] red green blue ka kd ks kt n       */
    double eye[3];           /* Scene.eye       scene_reader.py:151-152       */
    double ortho[4];         /* Scene.ortho     x0 y0 x1 y1                   */
    double ambient;          /* Scene.ambient                                 */
    double light_rgb[3];     /* Scene.light_color                             */
} pt_scene_desc;

/* Render parameters.  Pixel k = ix*height + iy is the reference's list order
 * (utils.py:64-69).  Rows: a launch renders the image rows iy with
 * row_begin <= iy < row_end and iy % row_step == row_phase, which covers
 * contiguous bands (row_step 1) and the interleaved bands used for
 * multi-GPU balance.  Output: image orientation, float32 (float64 with
 * PT_FLAG_OUT_F64) out[(height-1-iy)][ix][3] restricted to the launched rows,
 * in launch order (see pt_band_rows), one output row every out_row_stride
 * elements (0: packed, width*3) — a band can be written straight into its
 * rows of a whole frame (out = the frame's row of the band's top iy, stride =
 * row_step*width*3).  Values are the averaged radiance before make_image's
 * min-max normalisation (main.py:274-280).
 *
 * lanes_per_pixel: 0 lets the library choose the work-items per pixel of the
 * launch (from the launch's size and the device: one rank's band of an N-GPU
 * split gets more lanes per pixel than the whole frame); a power of two
 * <= min(64, spp) fixes it.  A pixel's samples are summed in an order that
 * follows its lane count, so two launches covering a pixel give bit-identical
 * values when they use the same lanes_per_pixel, and values within ~1e-15
 * relative of each other otherwise.                                        */
typedef struct pt_render_params {
    int32_t width, height;
    int32_t spp;             /* main.py -r                                     */
    int32_t bounces;         /* main.py -b                                     */
    uint64_t seed;           /* RNG key (SDL `seed`, unused by the reference) */
    uint32_t flags;          /* PT_FLAG_*                                      */
    int32_t rr_depth;        /* first bounce that may be terminated by RR     */
    int32_t row_begin, row_end, row_step, row_phase;
    int32_t sample_begin;    /* first sample index (spp-split renders)        */
    int32_t out_row_stride;  /* elements between output rows (0: width*3)     */
    int32_t lanes_per_pixel; /* 0: chosen per launch; else fixed (see above)  */
    int32_t reserved;        /* 0 */
} pt_render_params;

/* Work counters (PT_FLAG_COUNT); reference-semantics test counts are those
 * the reference loop would execute (shadow rays stop at the first occluding
 * object, main.py:42-55).                                                   */
typedef struct pt_stats {
    uint64_t closest_tests;   /* intersect calls of intersect_objects        */
    uint64_t shadow_tests;    /* intersect calls of compute_shadow_rays      */
    uint64_t ray_bounces;     /* non-None rays traced                        */
    uint64_t shading_points;  /* compute_color calls                         */
    uint64_t light_hits;
    uint64_t escapes;
    uint64_t f64_fallbacks;   /* single tests re-evaluated in f64 (filter)   */
    uint64_t f64_rescans;     /* closest-hit queries re-run fully in f64     */
    /* PT_FLAG_WALK_COUNT (wavefront renders of BVH scenes): the walk kernels'
     * work — queries taken, 4-wide node visits, BVH leaf units tested      */
    uint64_t shadow_queries, shadow_node_visits, shadow_leaf_units;
    uint64_t closest_queries, closest_node_visits, closest_leaf_units;
    /* PT_FLAG_KERNEL_TIMES (wavefront renders): summed HIP-event time (ms)
     * and launch count of each wavefront kernel                            */
    double shade_ms, shadow_ms, closest_ms;
    uint64_t shade_launches, shadow_launches, closest_launches;
    /* (v7) the shadow list's counting sort between the shade and the shadow
     * walks (its four kernels per step) */
    double sort_ms;
    uint64_t sort_launches;
} pt_stats;

typedef struct pt_scene pt_scene;

int pt_api_version(void);
const char* pt_last_error(void);
/* Content hash (16 hex digits) of the sources the library was compiled from
 * (the .h and .hip files of csrc/ and this header; pathtracerpython_amd/build.py).  The
 * Python binding refuses a library whose id is not the hash of the sources on
 * disk, and measurements name the loaded library's id.  (v6) */
const char* pt_build_id(void);

/* number of HIP devices visible to the library */
int pt_device_count(int32_t* count);

/* Upload a scene to the current HIP device.  Replaces Scene(path)'s role as
 * the thing the workers receive by pickle (main.py:201, :219). */
int pt_scene_create(const pt_scene_desc* desc, pt_scene** out);
/* Same, on HIP device `device` (the current device is left unchanged). */
int pt_scene_create_on(const pt_scene_desc* desc, int32_t device, pt_scene** out);
/* Same, with a thin lens (PT_FLAG_LENS; v7, additive).  The f32 filter's
 * "all" frame — the box every primary ray's origin lies in — is extended by
 * eye.x +- radius, eye.y +- radius before its centre, half extent and the
 * error bounds that grow with them are derived; the surface frame is
 * untouched.  Requires radius and focus_z finite, radius >= 0, eye[2] != 0 and
 * tau = (eye[2] - focus_z)/eye[2] finite and > 0 (the focal plane on the
 * screen's side of the eye), PT_EINVAL otherwise.  device -1: the current
 * device, as pt_scene_create.  lens == NULL: exactly pt_scene_create_on. */
typedef struct pt_lens {
    double radius, focus_z;
} pt_lens;
int pt_scene_create_lens(const pt_scene_desc* desc, int32_t device, const pt_lens* lens,
                         pt_scene** out);
void pt_scene_destroy(pt_scene* scene);

/* Number of rows a launch with these params renders. */
int pt_band_rows(const pt_render_params* p, int32_t* rows);

/* Whole loop main.py:186-280 for the selected rows.  out_rgb_dev is a DEVICE
 * pointer (rows*width*3 float32, or float64 with PT_FLAG_OUT_F64), written on
 * `stream` (a hipStream_t, or NULL for the null stream).  Asynchronous unless
 * stats are requested with PT_FLAG_COUNT; pt_last_kernel_ms() reads the
 * HIP-event time of the most recent launch. */
int pt_render_device(pt_scene* scene, const pt_render_params* p,
                     void* out_rgb_dev, void* stream, pt_stats* stats);

/* Same, synchronous, with a host output buffer (rows*width*3 elements, or
 * rows rows of out_row_stride elements). */
int pt_render(pt_scene* scene, const pt_render_params* p, void* out_rgb_host,
              pt_stats* stats);

/* Several GPUs from one process (SURVEY.md §8(b) pt_render_multi; the
 * reference's only parallelism is its process pool over rays,
 * main.py:197-231).  scenes[i] is a handle of the same scene created on its
 * own device (pt_scene_create_on).  The rows row_begin <= iy < row_end of p
 * (p->row_step must be 1) are dealt out interleaved: handle i renders the
 * rows with (iy - row_begin) % n == i, all devices concurrently, and each
 * band is copied with one strided device-to-host copy straight into its rows
 * of out_rgb_host ((row_end-row_begin) x width x 3, the layout pt_render
 * writes for the whole range; p->out_row_stride must be 0).  Bit-identical to
 * pt_render of the same range on one device when p->lanes_per_pixel is set
 * (the same value for both); with 0 each band's launch chooses its own
 * lanes per pixel and values agree to ~1e-15 relative (see
 * pt_render_params).  Synchronous.  On an error the devices already launched
 * are drained before it returns, so the handles and out_rgb_host are free
 * for reuse.  stats (optional) receives the per-device sums of every field
 * (PT_FLAG_COUNT / PT_FLAG_WALK_COUNT / PT_FLAG_KERNEL_TIMES renders then run
 * one device at a time). */
int pt_render_multi(pt_scene* const* scenes, int32_t n, const pt_render_params* p,
                    void* out_rgb_host, pt_stats* stats);

/* Kernel time (ms) of the last pt_render_device launch on this handle. */
int pt_last_kernel_ms(pt_scene* scene, float* ms);

/* Which path the handle's last launch took (v7, additive): a host-side record
 * without synchronisation, written by every pt_render_device, pt_render and
 * pt_accum_render(_stats) call that launches (pt_render_multi: each handle's
 * own); a call that launches nothing leaves it as it was. */
#define PT_PATH_NONE 0       /* no launch on this handle yet */
#define PT_PATH_SINGLE 1
#define PT_PATH_WAVEFRONT 2
typedef struct pt_launch_info {
    int32_t path;             /* PT_PATH_* of the handle's last launch */
    int32_t steps;            /* wavefront: shade launches issued; single kernel: 1 */
    int32_t lanes_per_pixel;  /* the split the launch used */
    uint32_t flags;           /* the launch's PT_FLAG_* */
} pt_launch_info;             /* 16 bytes */
int pt_last_launch_info(pt_scene* scene, pt_launch_info* info);

/* Radiance for caller-supplied rays (build extension; v7,
 * additive): the path loop of main.py:186-271 for any camera.  A ray record: */
typedef struct pt_ray {
    double o[3];             /* the primary ray's origin                      */
    double d[3];             /* its direction, any finite length != 0 (not
                                checked, see below)                           */
    uint32_t key;            /* the Philox pixel word of the record's draws   */
    uint32_t reserved;       /* 0 */
} pt_ray;                    /* 56 bytes */
/* THE RULE.  Sample s (absolute index: s = sample_begin + j, as for a frame)
 * of record i is the reference's sample of main.py:186-271 with three
 * substitutions:
 *  - the primary ray's origin is o;
 *  - its direction is d, used exactly where a frame's d0 is used (so it is
 *    normalised by the same code, and stays unnormalised where d0 does: the
 *    incoming direction of bounce 0);
 *  - eye = o wherever the sample reads the eye, the specular term of the
 *    bounce included.
 * The Philox pixel word of every draw of the sample is `key` (a frame's
 * k = ix*H + iy); record i's position in the batch plays no part.  An escape
 * contributes 0, a light hit light_rgb, per sample; bounces <= 0 gives 0.  The
 * result of a record is the mean over the spp samples; with out_S / out_Q, also
 * the per-channel sums S of the sample colours and Q of their squares, formed
 * sample by sample as an accumulator pass forms them (a whole path per
 * sample), and then the mean is S / spp.  The value depends on (seed, key, s,
 * o, d) only: not on the batch, its order, or — at a fixed lanes_per_pixel —
 * on how a record's samples are dealt to lanes (with lanes_per_pixel 0 the
 * library chooses from n_rays, and results agree to ~1e-15 relative).  Records
 * with the same key are allowed and share draws.  Without out_S / out_Q the
 * samples are summed as a frame's are, so the rays of a frame with the
 * frame's keys (o = eye, d = (x - ex, y - ey, 0 - ez), key = ix*H + iy) give
 * pt_render's pixels bit for bit at the same lanes per pixel — the lanes the
 * frame's launch really gave the pixel: on a scene without a BVH pt_render
 * gives the frame's top sixteenth of rows (iy >= H - ceil(H/16)) up to 8 times
 * the lanes of lanes_per_pixel where spp allows it (min(64, spp) caps them),
 * so those rows agree to ~1e-15 relative instead, unless spp leaves no room
 * (lanes_per_pixel = the largest power of two <= spp).  A ray that
 * crosses z = 0 going forward at p is the reference's primary ray of pixel k
 * on a descriptor with eye = o, H = 1, W = k + 1, ortho = (., p.y, p.x, .).
 *
 * A scene made for rays: pt_scene_create_rays sizes the f32 filter's "all"
 * frame for primary origins anywhere in box ({lo x, y, z, hi x, y, z}, finite,
 * lo <= hi) as well as the eye, as pt_scene_create_lens does for its disc.
 * box == NULL: exactly pt_scene_create_on; scenes made by the other entries
 * keep their records byte for byte.  A ray whose origin lies outside the
 * frame the scene was prepared for is answered all the same: its primary query
 * alone is decided in f64, as PT_FLAG_FORCE_F64 decides every query (the f32
 * bounds are never consulted outside the extent they were derived for); on a
 * scene made without a box that is every origin outside the box of the
 * triangles and the eye (the cube of its longest side about its centre).    */
int pt_scene_create_rays(const pt_scene_desc* desc, int32_t device, const double box[6],
                         pt_scene** out);
/* rays_dev: n_rays records in DEVICE memory.  out_rgb_dev: [n_rays][3] float32
 * (float64 with PT_FLAG_OUT_F64), in the records' order.  out_S_dev, out_Q_dev:
 * [n_rays][3] float64 each, both or neither (NULL).  p: width, height and the
 * row fields are ignored; spp >= 1, bounces, seed, sample_begin, rr_depth and
 * lanes_per_pixel (0, or a power of two <= min(64, spp)) apply.  Flags:
 * PT_FLAG_RR, PT_FLAG_FORCE_F64, PT_FLAG_OUT_F64 and PT_FLAG_RAYS_SINGLE; any
 * other bit is PT_EINVAL (PT_FLAG_AA, PT_FLAG_LENS, PT_FLAG_COUNT,
 * PT_FLAG_MEGAKERNEL and the stats flags among them), and so are a NULL ray
 * or output array with n_rays > 0, n_rays < 0 or >= 2^30, and a launch of
 * 2^32 work-items or more.  n_rays = 0 succeeds, writes nothing and leaves
 * the handle's last-launch record as it was.
 * ROUTING, by a frame's rule: on a scene with a BVH the launch goes through
 * the wavefront kernels (the ray forms of the shade, primary and final
 * kernels, pt_shade_rays.hip; the frames' walk and sort kernels): one primary
 * query per record, its hit cached, ceil(spp / lanes) x bounces + 2 shade
 * steps.  The single kernel k_render_rays takes the launch on a scene
 * without a BVH, with PT_FLAG_RAYS_SINGLE or PT_FLAG_FORCE_F64, on a tree
 * deeper than the walk stack, and at 2^29 path slots (n_rays x lanes) or
 * more.  The lanes per record come from one rule on both paths, and the two
 * paths agree bit for bit in the mean, S and Q.  A record whose origin lies
 * outside the frame has its primary query decided in f64 on either path.  The
 * wavefront buffers are the handle's, shared with its frames and grown on
 * demand: about 440 B per path slot (+ 48 B with out_S / out_Q) and 48 B per
 * record; a failed allocation is PT_ENOMEM (a batch is not chunked).
 * Asynchronous on `stream`; pt_last_kernel_ms covers the whole launch and
 * pt_last_launch_info tells the path.  The device form does not read
 * `reserved`.
 * Neither form checks o or d: a record whose d is zero or whose o or d is not
 * finite has a NaN direction or origin, every test against it fails as the
 * reference's comparisons do, and the record's value is unspecified (0, as an
 * escape, or NaN); no other record is affected and nothing is read or
 * written out of bounds.                                                      */
int pt_radiance_device(pt_scene* scene, const pt_ray* rays_dev, int64_t n_rays,
                       const pt_render_params* p, void* out_rgb_dev, double* out_S_dev,
                       double* out_Q_dev, void* stream);
/* Same, synchronous, on HOST arrays; a record with reserved != 0 is PT_EINVAL. */
int pt_radiance(pt_scene* scene, const pt_ray* rays, int64_t n_rays, const pt_render_params* p,
                void* out_rgb, double* out_S, double* out_Q);

/* Adaptive sampling to a noise target (v7, additive; build extension — the
 * reference spends -r samples on every pixel, main.py:186-271).  A pt_accum is
 * a device-resident accumulator of one (width, height) frame of `scene`.  Per
 * pixel e = (height-1-iy)*width + ix (image orientation) it holds
 *     S[e][3]  f64  sum of the pixel's sample colours,
 *     Q[e][3]  f64  per-channel sum of their squares (one sample colour is
 *                   what the reference adds to pixel_color_list per
 *                   rays_counter, main.py:269-271: a whole path),
 *     n[e]     u32  samples taken — always the sample indices 0..n-1,
 *     err[e]   f64  the error estimate of the last pt_accum_select,
 * and the active list of that select: u32 values of e, ascending, unique.
 * Error estimate (f64 throughout, in this order), for n >= 2 and channel c:
 *     m_c = S_c / n
 *     v_c = max(0, Q_c - S_c*S_c / n) / (n - 1)
 *     err = sqrt((v_r + v_g + v_b) / n) / (|m_r| + |m_g| + |m_b| + floor)
 * and err = +inf for n < 2.  A pixel is active iff
 *     n < min_spp || (err > tol && n < max_spp),
 * and a render pass adds k = min(step_spp, (n < min_spp ? min_spp : max_spp) - n)
 * samples, the indices n .. n+k-1, to each listed pixel.  The keyed RNG makes
 * sample s of a pixel the same draw whichever pass renders it, so a pixel that
 * stopped at n samples holds what a uniform render of n samples gives it
 * (to the sum order: ~1e-15 relative).  tol = 0 takes every pixel of non-zero
 * variance to max_spp; min_spp == max_spp is a uniform render that also
 * yields Q.  Requires 2 <= min_spp <= max_spp, step_spp >= 1, tol >= 0,
 * floor > 0 (PT_EINVAL otherwise).                                         */
typedef struct pt_adapt_params {
    double tol;              /* stop at err <= tol                            */
    double floor;            /* added to the mean's magnitude (dark pixels)   */
    int32_t min_spp;         /* every pixel gets at least this many samples   */
    int32_t max_spp;         /* the per-pixel budget                          */
    int32_t step_spp;        /* samples a pass adds per listed pixel          */
    int32_t reserved;        /* 0 */
} pt_adapt_params;

typedef struct pt_accum pt_accum;

/* An empty accumulator (n = 0 everywhere) on the scene's device.  It uses the
 * scene handle's launch ordering and shares its rule: one call at a time per
 * scene handle, accumulator calls included; launches are ordered after the
 * handle's previous launch whatever stream either was issued on.  Destroy it
 * before the scene. */
int pt_accum_create(pt_scene* scene, int32_t width, int32_t height, pt_accum** out);
void pt_accum_destroy(pt_accum* acc);
/* n = 0, S = Q = 0, err = +inf, empty list.  Asynchronous on `stream`. */
int pt_accum_reset(pt_accum* acc, void* stream);
/* err of every pixel and the active list (an ordered stream compaction: a
 * count per block, a scan, a scatter).  The list's length stays in device
 * memory; this call reads it back — the only host synchronisation of a pass —
 * into *n_active, with the samples the pass will add in *pass_samples
 * (either may be NULL). */
int pt_accum_select(pt_accum* acc, const pt_adapt_params* a, void* stream,
                    uint32_t* n_active, uint64_t* pass_samples);
/* One pass over the active list of the last pt_accum_select made with the
 * same `a` (when there is none since the last change of the accumulator, the
 * select runs first): k more samples for each listed pixel.  p describes the
 * whole frame: width and height the accumulator's, spp = a->max_spp,
 * row_begin 0, row_end height, row_step 1, row_phase 0, sample_begin 0,
 * out_row_stride 0, lanes_per_pixel 0, flags within PT_FLAG_RR |
 * PT_FLAG_FORCE_F64 | PT_FLAG_MEGAKERNEL | PT_FLAG_WALK_COUNT |
 * PT_FLAG_KERNEL_TIMES | PT_FLAG_AA | PT_FLAG_LENS (one value of PT_FLAG_AA
 * and one of PT_FLAG_LENS between resets, see the flags; PT_FLAG_LENS with
 * PT_FLAG_WALK_COUNT or PT_FLAG_KERNEL_TIMES is PT_EINVAL on either path);
 * anything else is PT_EINVAL.  Scenes with a BVH run
 * the pass through the wavefront kernels (shade, sort and walk steps over the
 * slots of the listed pixels) under pt_render_device's conditions, and
 * through the single kernel with PT_FLAG_MEGAKERNEL or PT_FLAG_FORCE_F64;
 * both use the same lanes per pixel, so S, Q and n are the same bit for bit.
 * Asynchronous on `stream` (after the select's read); pt_last_kernel_ms()
 * gives the pass's kernel time. */
int pt_accum_render(pt_accum* acc, const pt_render_params* p, const pt_adapt_params* a,
                    void* stream);
/* The same pass with stats (may be NULL): with PT_FLAG_WALK_COUNT /
 * PT_FLAG_KERNEL_TIMES in p->flags a wavefront pass fills the walk counters /
 * the per-kernel launch counts and times as pt_render_device does (and is
 * then synchronous); a single-kernel pass leaves them 0.  (v7, additive) */
int pt_accum_render_stats(pt_accum* acc, const pt_render_params* p, const pt_adapt_params* a,
                          void* stream, pt_stats* stats);
/* S / n (0 where n = 0) into a framebuffer of pt_render_device's layout for
 * the whole frame: height*width*3 float32, or float64 with PT_FLAG_OUT_F64 in
 * flags (no other flag).  Asynchronous on `stream`. */
int pt_accum_resolve_device(pt_accum* acc, uint32_t flags, void* out_rgb_dev, void* stream);
/* Synchronous copy-out after the handle's last launch; NULL pointers are
 * skipped.  S, Q: [height*width][3] f64; n: [height*width] u32; err:
 * [height*width] f64; list: up to list_cap entries of the last select's list,
 * *list_len its length (list needs list_len). */
int pt_accum_read(pt_accum* acc, double* S, double* Q, uint32_t* n, double* err,
                  uint32_t* list, uint32_t list_cap, uint32_t* list_len);

/* A band on the accumulator (v7, additive): the select, and with it every
 * pass, is restricted to the rows pt_band_rows() names — row_begin <= iy <
 * row_end with iy % row_step == row_phase — so that N accumulators, one per
 * device, can each run the pass loop of their own rows with no exchange until
 * the end (a pixel's trajectory through the passes depends on nothing but its
 * own S, Q, n; the RNG key is (seed, pixel, sample, bounce)).  The default
 * band is (0, height, 1, 0) with lanes_per_pixel 0: the whole frame, exactly
 * the accumulator without a band.  The allocations stay whole-frame; only the
 * work is restricted.
 *
 * Select on a band: the grid covers the band's rows*width pixels; band pixel b
 * is (j = b / width, ix = b % width) with j counting the band's rows top-first
 * (iy descending), so e = (height-1-iy)*width + ix ascends with b and the list
 * stays ascending and unique.  With the default band b == e.  err is written
 * only inside the band; a band with no rows launches nothing and selects
 * (0, 0).
 *
 * lanes_per_pixel = L > 0: a pass uses
 *     split = min(L, largest power of two <= min(kmin, 64))
 * lanes per pixel (kmin: the smallest k of a listed pixel) instead of the
 * library's own choice, which depends on the list's length and so on the band.
 * Why a fixed L makes a banded run bit-identical to the whole-frame run: in a
 * run that starts from an empty accumulator every active pixel is listed in
 * every pass (an active pixel that is not rendered stays active), so all
 * active pixels share one n and therefore one k = kmin — in the whole-frame
 * run and in every band alike, pass by pass.  A fixed L then gives every pixel
 * the same lane count, hence the same samples per lane and the same xor-order
 * sum of the lanes' partial S and Q, wherever it is rendered.  With L = 0 the
 * lane counts may differ between the bands and the sums agree to the sum order
 * (~1e-15 relative); n is the same either way.
 *
 * pt_accum_render keeps its contract: the band and the lane count live on the
 * accumulator, not in pt_render_params (whose row_* and lanes_per_pixel fields
 * must stay at the whole-frame values there). */
typedef struct pt_accum_band {
    int32_t row_begin, row_end, row_step, row_phase;  /* the rows pt_band_rows() names */
    int32_t lanes_per_pixel;  /* 0: chosen per pass as today; else a power of two <= 64 */
    int32_t reserved;         /* 0 */
} pt_accum_band;              /* 24 bytes */
/* Requires row_step >= 1, 0 <= row_phase < row_step, 0 <= row_begin <= row_end
 * <= height, lanes_per_pixel 0 or a power of two <= 64, reserved 0; anything
 * else is PT_EINVAL and leaves the accumulator and its band as they were.  May
 * be called at any time; it invalidates the last select's list and changes
 * nothing else.  While the band's rows are not the whole frame,
 * pt_accum_features, pt_accum_read_features and pt_accum_denoise_device return
 * PT_EINVAL (the neighbour rows are empty); pt_accum_resolve_device and
 * pt_accum_read work on the whole frame as ever. */
int pt_accum_set_band(pt_accum* acc, const pt_accum_band* band);

/* Band tiles: the state of a band's P = rows*width pixels as one flat buffer,
 * the pixels top-first (ascending e), in four sections:
 *     S    [P][3] f64  at byte 0
 *     Q    [P][3] f64  at byte 24 P
 *     err  [P]    f64  at byte 48 P
 *     n    [P]    u32  at byte 56 P
 * 60 P bytes (pt_accum_tile_bytes; rows >= 0, width > 0).  One flat buffer so
 * that it crosses devices with a 1-D copy.
 * pt_accum_export_band_device packs the accumulator's own band into tile_dev;
 * pt_accum_import_band_device scatters a tile into the rows of `band` (its
 * lanes_per_pixel is ignored), overwriting S, Q, err and n there and
 * invalidating the list; it does not change the accumulator's own band.
 * tile_dev is 8-byte aligned device memory of the accumulator's device.  One
 * HBM-bound kernel each; asynchronous on `stream`, ordered on the scene handle
 * like every accumulator launch.  One whole-frame accumulator out of N banded
 * ones: import the tiles of bands 1..N-1 into band 0's accumulator, then set
 * the default band — it can be read, resolved, denoised or run further. */
int pt_accum_tile_bytes(int32_t width, int32_t rows, uint64_t* bytes);
int pt_accum_export_band_device(pt_accum* acc, void* tile_dev, void* stream);
int pt_accum_import_band_device(pt_accum* acc, const pt_accum_band* band,
                                const void* tile_dev, void* stream);
/* The host counterpart of pt_accum_read, synchronous: whole-frame S, Q
 * ([height*width][3] f64) and n ([height*width] u32) — all three required —
 * replace the accumulator's; err becomes +inf everywhere and the list is
 * invalidated.  A run continues from the written state as from its own. */
int pt_accum_write(pt_accum* acc, const double* S, const double* Q, const uint32_t* n);

/* Ray accumulators (v7, additive): adaptive sampling for caller-supplied rays.
 * A pt_accum of width x height elements, n = width*height with 1 <= n < 2^30
 * (PT_EINVAL otherwise), whose element e belongs to ray record e — not to a
 * pixel of the scene's camera.  rays_dev: the n records in DEVICE memory; they
 * are copied at create, so the caller's buffer may go away on return.  The
 * copy runs on a stream of the accumulator's own and is not ordered after any
 * stream of the caller's: the records must be complete in device memory (the
 * work that wrote them synchronised) before the call.  The
 * device form does not read `reserved`, as pt_radiance_device does not.  A
 * flat batch uses height = 1; an image uses its own shape with the records in
 * image orientation, e = (height-1-iy)*width + ix.
 * THE RULE.  A pass adds the samples n[e] .. n[e]+k-1 of record e to each
 * listed element, k as for a frame accumulator; each of them is THE RULE of
 * pt_radiance with s the absolute sample index, formed sample by sample (a
 * whole path per sample).  The value depends on (seed, key, s, o, d) only: not
 * on the record's position, the list, the pass that takes the sample, or — at a
 * fixed lanes per record — on how the samples are dealt to lanes.  The rays of
 * a frame with the frame's keys, in image orientation, therefore give a frame
 * accumulator's S, Q and n bit for bit at the same lanes per record.
 * On a ray accumulator pt_accum_reset, _select, _read, _write,
 * _resolve_device, _set_band, _tile_bytes, _export_band_device,
 * _import_band_device and _destroy mean what they mean on a frame accumulator
 * and run the same code (a "row" is a row of the width x height shape); in
 * pt_accum_band, lanes_per_pixel is lanes per record, with the same
 *     split = min(L, largest power of two <= min(kmin, 64)).
 * pt_accum_render(_stats): p->width and p->height are the accumulator's,
 * spp = a->max_spp, and the row fields, sample_begin, out_row_stride and
 * lanes_per_pixel stay at their whole-frame values.  Flags: PT_FLAG_RR,
 * PT_FLAG_FORCE_F64 and PT_FLAG_RAYS_SINGLE (accepted, no effect yet: reserved
 * for the wavefront form); any other bit — PT_FLAG_AA, PT_FLAG_LENS,
 * PT_FLAG_MEGAKERNEL, PT_FLAG_COUNT, PT_FLAG_WALK_COUNT, PT_FLAG_KERNEL_TIMES
 * and PT_FLAG_OUT_F64 among them — is PT_EINVAL with a message naming it, and
 * so is a launch of 2^32 work-items or more.  The pass is one launch of the
 * list kernel over ray records (k_render_rays_list, pt_rays_list.hip) on every
 * scene, a scene with a BVH included; pt_last_launch_info reports
 * PT_PATH_SINGLE, the lanes per record and the flags; stats stay 0.  A record
 * whose origin lies outside the frame the scene was prepared for
 * (pt_scene_create_rays) has its primary query decided in f64.
 * pt_accum_features traces each record's ray, o and d used as a pass uses them
 * (outside the frame: in f64); tri, obj, N and P keep their layout, so
 * pt_accum_read_features and pt_accum_denoise_device work unchanged on the
 * width x height shape (whole band only): the filter reads S, Q, n and the
 * features, nothing of the camera.  Neighbours in the filter are neighbours in
 * the shape, which is meaningful for an image of records. */
int pt_accum_create_rays(pt_scene* scene, const pt_ray* rays_dev, int32_t width, int32_t height,
                         pt_accum** out);

/* Denoising an adaptive render on the device (additive; build extension — the
 * reference has no filter).  An edge-avoiding a-trous filter over the frame,
 * guided by the per-pixel variance of the mean (from an accumulator's S, Q, n)
 * and by the first hit of each pixel's primary ray.  It changes no sample: it
 * produces a second, filtered frame.  Pixel e = row*W + col in image
 * orientation (row = H-1-iy, col = ix).  Everything is f64, each operation
 * rounded on its own, in exactly this order (IEEE division and sqrt, no fma).
 *
 * Inputs per pixel: colour c[3], variance of the mean v[3], features obj
 * (i32), N[3], P[3].  From an accumulator:
 *     n >= 2:  c = S/n,  v = (max(0, Q - S*S/n)/(n-1))/n
 *     n == 1:  c = S,    v = c*c      (variance unknown: lean on the neighbours)
 *     n == 0:  c = v = 0
 * Constants: A = (0.2126, 0.7152, 0.0722), B_k = A_k*A_k,
 * H5 = (1/16, 1/4, 3/8, 1/4, 1/16), G = (1/4, 1/2, 1/4).  max(0, x) is
 * x > 0 ? x : 0.
 * Iteration i = 0 .. iters-1, stride s = 2^i, reading (c, v), writing (c', v'):
 *  1. l = (A0*c0 + A1*c1) + A2*c2, vl = (B0*v0 + B1*v1) + B2*v2 at every pixel.
 *  2. At pixel p: vf = sum of (G[dy+1]*G[dx+1]) * vl[clamped (row+dy, col+dx)],
 *     dy outer and dx inner over -1..1, accumulated from 0.0;
 *     dl = sigma_l*sqrt(vf) + eps.
 *  3. Taps dy outer, dx inner over -2..2 at q = (row+dy*s, col+dx*s).  A tap
 *     outside the frame, or with obj[q] != obj[p], is skipped.  Otherwise
 *         w = H5[dy+2]*H5[dx+2]
 *         if obj[p] >= 0:
 *             nd = max(0, (Np0*Nq0 + Np1*Nq1) + Np2*Nq2); nd = nd*nd, normal_sq times
 *             D = Pq - Pp; dist = sqrt((D0*D0 + D1*D1) + D2*D2)
 *             pd = |(Np0*D0 + Np1*D1) + Np2*D2|
 *             xz = dist > 0 ? pd/(dist*sigma_z) : 0
 *             wz = max(0, 1 - xz); wz = wz*wz;  w = (w*nd)*wz
 *         xl = |l[q] - l[p]| / dl
 *         w = w * (1/((1 + xl) + 0.5*(xl*xl)))
 *         num_k += w*c[q][k];  vnum_k += (w*w)*v[q][k];  den += w
 *  4. c'_k = num_k/den, v'_k = vnum_k/(den*den) (the centre tap makes den > 0).
 * Requires 1 <= iters <= 8, 0 <= normal_sq <= 8, sigma_l > 0, sigma_z > 0,
 * eps > 0, reserved 0 (PT_EINVAL otherwise); frames of 2^30 pixels or more
 * are refused.  N of a hit pixel is a unit vector (the centre tap's weight is
 * (N.N)^(2^normal_sq)).  Defaults of the Python layer: iters 5, sigma_l 2.0,
 * sigma_z 0.1, eps 1e-10, normal_sq 5.                                       */
typedef struct pt_denoise_params {
    double sigma_l;          /* luminance stop, in standard deviations        */
    double sigma_z;          /* plane-distance stop, relative to the tap's distance */
    double eps;              /* added to the luminance stop's scale           */
    int32_t iters;           /* iterations; iteration i has stride 2^i        */
    int32_t normal_sq;       /* the normal stop is (Np.Nq)^(2^normal_sq)      */
    int32_t reserved;        /* 0 */
} pt_denoise_params;         /* 40 bytes (4 of tail padding) */

/* The filter on caller-provided DEVICE arrays of the current device, scene-free
 * like pt_image_u8_device: c, v, N, P [height*width][3] f64, obj
 * [height*width] i32 (read-only); out_rgb and out_var (may be NULL)
 * [height*width][3] float32, or float64 with PT_FLAG_OUT_F64 in flags (the
 * only flag).  The call owns its scratch: two (c, v) frames, 96 B per pixel,
 * allocated and freed on `stream` (stream-ordered).  Asynchronous on `stream`. */
int pt_denoise_device(int32_t width, int32_t height, const pt_denoise_params* params,
                      const double* c, const double* v, const int32_t* obj, const double* N,
                      const double* P, uint32_t flags, void* out_rgb, void* out_var, void* stream);
/* Same, synchronous, with host arrays. */
int pt_denoise(int32_t width, int32_t height, const pt_denoise_params* params, const double* c,
               const double* v, const int32_t* obj, const double* N, const double* P,
               uint32_t flags, void* out_rgb, void* out_var);

/* First-hit features of the accumulator's frame, one primary ray per pixel
 * (the ray a render builds; closest hit as pt_intersect_objects finds it):
 * tri (i32, -1 for an escape), obj = tri_obj[tri] (the light is n_obj, an
 * escape -1), N = tri_n[tri] as the scene descriptor holds it (no flip, no
 * renormalisation), P = the f64 hit point; N = P = 0 for an escape.  Computed
 * once per accumulator and kept (a second call does nothing); allocated at
 * the first call, 56 B per pixel, so an accumulator that is never denoised
 * costs nothing more.  Asynchronous on `stream`. */
int pt_accum_features(pt_accum* acc, void* stream);
/* Synchronous copy-out (computes the features first when missing); NULL
 * pointers are skipped.  tri, obj: [height*width] i32; N, P:
 * [height*width][3] f64. */
int pt_accum_read_features(pt_accum* acc, int32_t* tri, int32_t* obj, double* N, double* P);
/* The filtered frame of the accumulator's present state: moments -> (c, v),
 * the features when missing, params->iters iterations, then out_rgb_dev and
 * out_var_dev (may be NULL) as pt_denoise_device writes them; flags:
 * PT_FLAG_OUT_F64 only.  S, Q, n, err and the list are left untouched, and a
 * run continues after it as if it had not happened.  Ordered on the scene
 * handle like every accumulator launch.  The accumulator keeps the scratch
 * from the first call on: two (c, v) frames, 96 B per pixel, beside the 56 B
 * per pixel of features — 152 B per pixel, 2.6 GB at 4096 x 4096.
 * Asynchronous on `stream`. */
int pt_accum_denoise_device(pt_accum* acc, const pt_denoise_params* params, uint32_t flags,
                            void* out_rgb_dev, void* out_var_dev, void* stream);

/* Measurement hook (scripts/bench_denoise.py).  While enabled, a denoise call
 * records a HIP event around each of its launches, waits for them (the call
 * is then synchronous) and keeps the times in ms: k_accum_moments (the
 * accumulator form only), each iteration, the final store.  The call sets the
 * switch and copies out the times of the last timed denoise: up to cap values
 * into ms (may be NULL with cap 0), their number into *n (may be NULL).
 * Process-wide; off by default. */
int pt_denoise_times(int32_t enable, float* ms, int32_t cap, int32_t* n);

/* Batched replacement of intersect_objects (main.py:83-122).
 * rays: [n][6] f64 (origin, direction — direction need not be normalised).
 * out_tri [n]: closest triangle index or -1 (None); out_p [n][3]: hit point.
 * The light flag of the reference is out_tri >= n_obj_tri. */
int pt_intersect_objects(pt_scene* scene, const double* rays, int64_t n,
                         int32_t* out_tri, double* out_p);

/* Batched replacement of compute_color (main.py:142-145 + :23-80) with the
 * 12 light-sampling uniforms given explicitly per point (slots 0..11).
 * obj [n]: object index; point [n][3]; normal [n][3]; u [n][12];
 * out_rgb [n][3] f64. */
int pt_compute_color(pt_scene* scene, const int32_t* obj, const double* point,
                     const double* normal, const double* u, int64_t n,
                     double* out_rgb);

/* Frame assembly after the multi-GPU gather (replaces the
 * reference's collection of Pool results, main.py:224-231): tiles_dev is the
 * gathered (world, max_rows, width, 3) array whose band r is what
 * pt_render_device writes for row_step = world, row_phase = r over the whole
 * image (rows iy % world == r, top-first; max_rows >= ceil(height / world));
 * out_dev receives the (height, width, 3) framebuffer in image orientation.
 * Elements are float32, or float64 with PT_FLAG_OUT_F64 in flags.
 * Asynchronous on `stream`. */
int pt_assemble_bands_device(const void* tiles_dev, int32_t world, int32_t max_rows,
                             int32_t width, int32_t height, uint32_t flags, void* out_dev,
                             void* stream);

/* Host frames (the metric's framebuffer ends in host
 * memory; §8(e): the N ranks' bands make one frame).  The reference collects
 * the pool workers' colours into the parent's list through pipes
 * (main.py:204, :224-231); here each GPU writes its band straight into its
 * rows of one frame in page-locked host memory — shared by the rank
 * processes of one node (e.g. a /dev/shm mapping) — through a band render
 * with out = pt_host_map's device address of the band's first row and
 * out_row_stride = row_step*width*3, so the framebuffer crosses PCIe while the
 * kernel runs, each GPU over its own link.  Completion is a flag per rank in
 * the same memory: pt_signal writes it on the render's stream after the
 * render (system-scope release, so the band's stores are visible first), the
 * consumer waits for all flags with pt_wait_flags.
 *
 * pt_host_map page-locks [host, host+bytes) (caller-owned, page-aligned, e.g.
 * an mmap) for every device of the process and returns the address kernels
 * use for it; pt_host_unmap releases it (after the work using it is done). */
int pt_host_map(void* host, uint64_t bytes, void** dev_ptr);
int pt_host_unmap(void* host);
/* After all work queued on `stream` so far: *flag_dev = value (64-bit store,
 * system scope, release).  flag_dev: a pt_host_map address or device memory. */
int pt_signal(uint64_t* flag_dev, uint64_t value, void* stream);
/* Host: spin until flags[i * stride] >= value for i < n (relaxed loads, then
 * an acquire fence), or PT_ETIMEOUT after timeout_s seconds. */
int pt_wait_flags(const uint64_t* flags, int32_t n, int32_t stride, uint64_t value, double timeout_s);

/* Image finalisation of make_image (utils.py:150-161) on the device:
 * global min over the whole height x width x 3 array, shift, divide by the
 * shifted maximum, x255, truncate to uint8 — in f64, as numpy does (a NaN
 * anywhere, or a constant image, gives 0s like numpy's cast on x86).
 * fb: a full framebuffer as pt_render* writes it (image orientation, f32, or
 * f64 with PT_FLAG_OUT_F64 in flags); out: height*width*3 uint8 in the same
 * layout, which is make_image's array for the square images the reference
 * supports (for width != height its placement, utils.py:154-156, indexes out
 * of range).  The _device form is asynchronous on `stream`. */
int pt_image_u8_device(const void* fb_dev, int32_t width, int32_t height, uint32_t flags,
                       void* out_u8_dev, void* stream);
int pt_image_u8(const void* fb_host, int32_t width, int32_t height, uint32_t flags,
                uint8_t* out_u8_host);

/* Native OBJ reader (host only, no GPU needed) with the semantics of the
 * reference's Obj (scene_reader.py:49-104, vector.py:143-173): comment and
 * token rules, `v` / `f` records, negative indices, fan triangulation, and
 * the per-triangle normal and area computed in the reference's operation
 * order (bit-identical doubles).  Other commands are skipped; their raw line
 * byte ranges are returned so a caller can report them as the reference
 * prints them.  Returns PT_EUNSUPPORTED for inputs it does not mirror byte
 * for byte (e.g. "1/2/3" face tokens, hex or underscore numbers, vertices
 * with other than 3 coordinates, out-of-range indices, a zero-area
 * triangle): the caller then falls back to the Python reader, which raises
 * what the reference raises.  The mesh is owned by the library until
 * pt_mesh_free. */
typedef struct pt_mesh {
    int64_t n_vert, n_tri, n_skip;
    const double* vert;       /* [n_vert][3] */
    const int64_t* face;      /* [n_tri][3] vertex indices as Obj.faces holds them */
    const double* tri_v;      /* [n_tri][3][3] */
    const double* tri_n;      /* [n_tri][3] */
    const double* tri_area;   /* [n_tri] */
    const int64_t* skip_off;  /* [n_skip] byte offset of each skipped line */
    const int64_t* skip_len;  /* [n_skip] its length */
} pt_mesh;
int pt_obj_load(const char* path, pt_mesh** out);
void pt_mesh_free(pt_mesh* mesh);

/* Test hook (v6): the next pt_render_multi calls fail with PT_EHIP while
 * dealing band `multi_band`, after bands 0..multi_band-1 were launched (the
 * error path's drain); -1 (the default) turns it off.  Process-wide. */
int pt_test_fault_inject(int32_t multi_band);

#ifdef __cplusplus
}
#endif
#endif /* PT_CAPI_H */
