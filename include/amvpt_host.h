/*
 * amvpt_host.h -- C entry points of libamvpt_host.so, the Mitsuba-style host
 * framework around the hot path (XML scene subset, Properties, plugin
 * registry, MVPathIntegrator / PathIntegrator::render()).
 *
 * These mirror what the reference exposes to its front-ends:
 *   amvpt_host_load_file / _load_string  <- xml::load_file / load_string
 *                                           (src/core/xml.cpp; mitsuba_render.cpp:347)
 *   amvpt_host_render                    <- Integrator::render(scene, sensor_index, seed,
 *                                           spp, develop, evaluate)  integrator.cpp:30-42,
 *                                           dispatching to MVPathIntegrator::render mvpath.cpp:7-278
 *   amvpt_host_write_exr                 <- Film::write (hdrfilm.cpp, OpenEXR float32)
 *   amvpt_host_guides                    <- the aov integrator's position / geo_normal / shape_index
 *                                           (src/integrators/aov.cpp:245-300; see amvpt_guides.h)
 *   amvpt_host_denoise_stream            <- nothing: the reference has no denoiser (see amvpt_denoise.h)
 *   amvpt_host_display / _write_png     <- Program::display_image(screenshot) + Bitmap::write
 *                                           (src/mitsuba/program.cpp:199-276)
 *   amvpt_host_read_presets / _write_presets <- Preset::import_file / export_file (src/mitsuba/preset.h)
 *   amvpt_host_parse_fov / _perspective_projection
 *                                        <- parse_fov sensor.cpp:163-214,
 *                                           perspective_projection sensor.h:319-356
 * Errors: non-zero return + amvpt_host_last_error() carrying the reference's
 * Throw() message text.
 */
#ifndef AMVPT_HOST_H
#define AMVPT_HOST_H

#include "amvpt.h"
#include "amvpt_display.h"
#include "amvpt_guides.h"
#include "amvpt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amvpt_host_scene amvpt_host_scene;

const char *amvpt_host_last_error(void);

/* Load a scene; defines are `-D key=value` substitutions for <default>/$key. */
amvpt_host_scene *amvpt_host_load_file(const char *path, const char *const *keys,
                                       const char *const *values, int n_defines);
amvpt_host_scene *amvpt_host_load_string(const char *xml, const char *const *keys,
                                         const char *const *values, int n_defines);
void amvpt_host_scene_free(amvpt_host_scene *scene);

/* Film geometry of a sensor: quilt width/height, developed channels (3 or 4). */
int amvpt_host_film_info(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t *width,
                         uint32_t *height, uint32_t *channels, uint32_t *sample_count);
uint32_t amvpt_host_sensor_count(amvpt_host_scene *scene);

/*
 * Integrator::render(scene, sensor, seed, spp, develop=true).  Writes the developed
 * H x W x channels image to out_host (or the raw ImageBlock H x W x (4|5) when
 * raw != 0).  spp = 0 uses the sampler's sample_count.  Runs on the current HIP device.
 */
int amvpt_host_render(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                      int raw, float *out_host, amvpt_counters *counters);

/*
 * amvpt_host_render on a caller stream (hipStream_t; NULL: the default stream).  Both run through
 * amvpt_render_ex with explicit default options (no process-global knob), keep the device scene
 * (BVH build + upload) and the film / image buffers on the host scene per device for the next frame,
 * and serialise renders of one host scene (its cached buffers); renders of different host scenes from
 * different threads are independent.  Returns once the image is in out_host.
 */
int amvpt_host_render_stream(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                             int raw, float *out_host, void *stream, amvpt_counters *counters);
/* amvpt_host_render's cache counters: device-scene creations, buffer allocations, renders */
int amvpt_host_render_stats(amvpt_host_scene *scene, uint64_t *scene_creates, uint64_t *buffer_allocs,
                            uint64_t *renders);

/*
 * Integrator::render over n_devices GPUs of one node, one host thread per device.
 * View groups, when they divide among the devices (C5): devices[r] renders the lanes of its groups'
 * quilt tiles into a film window (tiles + filter border), the windows and overflow cells go to
 * devices[0] (ncclSend / ncclRecv) and are summed into the ImageBlock there (amvpt_film_accumulate).
 * Otherwise lane bands: devices[r] renders amvpt_host_lane_shard(L, r, n_devices) of every pass into
 * its own RGBW ImageBlock and the blocks are summed onto devices[0] with one ncclReduce.  Developed on
 * devices[0].  The adaptive fill's per-run count exchange runs between the threads (per-call option).
 * Communicators, per-device scenes and films are cached on the scene for the next frame.  The image
 * equals amvpt_host_render's up to float summation order.  Counters: lane statistics summed, times of
 * the slowest device.  A list naming ONE device several times is a shared-device rehearsal (one rank per
 * entry on that device, the films summed on it with amvpt_film_accumulate instead of RCCL; adaptive renders
 * are refused there, their count exchange needs concurrent renders); other repeated devices are an error.
 */
int amvpt_host_render_multi(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                            int raw, const int *devices, int n_devices, float *out_host,
                            amvpt_counters *counters);

/* [begin, end) of rank's contiguous lane range (sizes differ by at most one; amvpt.dist.lane_shard) */
void amvpt_host_lane_shard(uint64_t lanes, uint32_t rank, uint32_t world, uint64_t *begin, uint64_t *end);

/* The view-group partition of amvpt_host_render_multi (amvpt.dist.view_group_partition): rank's lane
 * rectangle and film window {x0, y0, width, height}; returns 1, or 0 when the view groups do not
 * divide among `world` devices as rectangles of quilt tiles (lane bands are used then). */
int amvpt_host_view_group_partition(const amvpt_params *params, uint32_t rank, uint32_t world, uint32_t *rect,
                                    uint32_t *window);

/* render_multi's per-scene cache (communicators, per-device scene copies, streams, films): how many
 * scene creations, communicator initialisations and completed multi-GPU renders it has seen. */
int amvpt_host_multi_stats(amvpt_host_scene *scene, uint64_t *scene_creates, uint64_t *comm_inits, uint64_t *renders);

/*
 * Test hook (CPU, no device): amvpt_host_render_multi's rank coordination (host/ranks.h: phase barriers,
 * the in-process count exchange and its abort) with n rank threads that each make `passes` count
 * exchanges in the render phase; rank fail_rank fails in phase fail_phase (0 setup, 1 render before its
 * exchanges, 2 render between them, 3 render after them, 4 before the gather, 5 finish; -1 none).
 * Returns 0 when every rank succeeded, 1 with the reported (first own) failure in
 * amvpt_host_last_error(), 2 if an exchange returned a wrong prefix.  Never leaves a thread blocked.
 */
int amvpt_host_test_ranks(int n, int passes, int fail_rank, int fail_phase);

/*
 * The exact descriptors render() hands to the C-ABI (for the parity tests: the oracle
 * consumes the same scene, views and params).  Pointers stay valid until the scene is freed.
 */
int amvpt_host_describe(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                        const amvpt_scene_desc **scene_desc, const amvpt_view_desc **views,
                        amvpt_params *params);

/* Text summary of the integrator (Integrator::to_string). */
const char *amvpt_host_integrator_string(amvpt_host_scene *scene);

/* OpenEXR (uncompressed float32 scanlines) writer / reader: channels 3 (RGB) or 4 (RGBA). */
int amvpt_host_write_exr(const char *path, const float *data, uint32_t width, uint32_t height,
                         uint32_t channels);
int amvpt_host_read_exr(const char *path, float *data, uint32_t width, uint32_t height,
                        uint32_t channels);

/*
 * Interleaved float32 channels (height x width x channels) under caller-given names, e.g. R, G, B, Z, N.X, ..., id.
 * The file stores them in the byte order of their names, as the format requires; the reader hands them back in the
 * caller's order, whatever that is.  Names are 1 to 31 bytes and unique; the reader needs the file to hold exactly
 * the named channels.  amvpt_host_write_exr is the same writer under the names R, G, B[, A] (or Y).
 */
int amvpt_host_write_exr_channels(const char *path, const float *data, uint32_t width, uint32_t height,
                                  uint32_t channels, const char *const *names);
int amvpt_host_read_exr_channels(const char *path, float *data, uint32_t width, uint32_t height,
                                 uint32_t channels, const char *const *names);

/*
 * Guide buffers of a sensor (amvpt_guides.h) on the current device: guides_host receives height x width x 8
 * float32 (shape index or -1, geometric normal, hit point, view index per quilt pixel), depth_host height x width
 * float32 (planar depth, +inf on a miss).  Either pointer may be NULL.  Runs on the device scene
 * amvpt_host_render caches for the current device (created on first use: a guides call after a render creates no
 * second one, see amvpt_host_render_stats) and does not touch the cached film or image.
 */
int amvpt_host_guides(amvpt_host_scene *scene, uint32_t sensor_index, float *guides_host, float *depth_host);

/*
 * The display stage (amvpt_display.h; the reference's front end, src/mitsuba/program.cpp:199-276): render ->
 * develop -> 8-bit sRGB quilt -> lenticular image of dst_w x dst_h, on the scene's cached device buffers and the
 * current device, with one download at the end: out_host_u8 receives dst_h x dst_w x 3 bytes.  preset NULL:
 * amvpt_host_preset_for_scene's.  quilt != 0 resamples the whole quilt instead; nearest != 0 picks texels instead
 * of the bilinear blend.  The stage reads the cached film and never writes it.  _stream runs on a caller stream
 * (hipStream_t; NULL: the default stream), as amvpt_host_render_stream does.
 */
int amvpt_host_display(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                       const amvpt_display_preset *preset, int quilt, int nearest, uint32_t dst_w, uint32_t dst_h,
                       uint8_t *out_host_u8, amvpt_counters *counters);
int amvpt_host_display_stream(amvpt_host_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                              const amvpt_display_preset *preset, int quilt, int nearest, uint32_t dst_w,
                              uint32_t dst_h, uint8_t *out_host_u8, void *stream, amvpt_counters *counters);

/*
 * The stage alone, without a render: sRGB quilt and display image of the developed frame that the last
 * amvpt_host_render* (raw == 0) or amvpt_host_display* of this sensor left on the current device -- what the
 * reference's front end does when a preset slider moves (program.cpp:200, m_update_view).  An error when no such
 * frame is cached.  Renders are not bit-reproducible (float atomics), so this is also how one frame is shown twice.
 */
int amvpt_host_redisplay_stream(amvpt_host_scene *scene, uint32_t sensor_index, const amvpt_display_preset *preset,
                                int quilt, int nearest, uint32_t dst_w, uint32_t dst_h, uint8_t *out_host_u8,
                                void *stream);

/*
 * The denoiser (amvpt_denoise.h) on the current device and a caller stream (hipStream_t; NULL: the default stream).
 * image_host NULL: the input is the developed frame that the last amvpt_host_render* (raw == 0) or
 * amvpt_host_display* of this sensor left on the device (an error when none is cached); otherwise image_host
 * (height x width x developed channels float32, amvpt_host_film_info's) is uploaded and filtered.  The guide
 * records come from amvpt_guides on the device scene amvpt_host_render caches (created on first use: a call after a
 * render creates no second one, see amvpt_host_render_stats).  params is required; sigma_plane is in world units.
 * out_host (NULL: nothing is downloaded) receives the filtered image.  replace != 0: the filtered image also becomes
 * the cached developed frame, so that amvpt_host_redisplay_stream shows it.  The cached film is not touched.
 * amvpt_host_render_multi has no denoise path; a view-group rank may run amvpt_denoise over the rectangle of its own
 * whole tiles and gets this entry's result there, because no tap crosses a view.
 */
int amvpt_host_denoise_stream(amvpt_host_scene *scene, uint32_t sensor_index, const amvpt_denoise_params *params,
                              const float *image_host, int replace, float *out_host, void *stream);

/* The default preset (LKG4x8) with `grid` set from the sensor's grid_x / grid_y; a batch sensor gives n x 1. */
int amvpt_host_preset_for_scene(amvpt_host_scene *scene, uint32_t sensor_index, amvpt_display_preset *preset);

/*
 * The reference's presets.csv (preset.h:19-57), one preset per line:
 *   name;center;focus;pitch;tilt;subp;view0;view1;grid0;grid1;flip_rgb
 * Floats are written with nine significant digits, so that writing then reading gives the same values (the
 * reference writes six and reads any number).  read fills at most `capacity` entries and sets *count to the
 * number of presets in the file; names longer than 63 bytes are cut.
 */
typedef struct amvpt_host_named_preset {
    char name[64];
    amvpt_display_preset preset;
} amvpt_host_named_preset;
int amvpt_host_read_presets(const char *path, amvpt_host_named_preset *presets, uint32_t capacity, uint32_t *count);
int amvpt_host_write_presets(const char *path, const amvpt_host_named_preset *presets, uint32_t count);

/* PNG writer, 8-bit RGB (height x width x 3 bytes): stored deflate blocks, no compression library. */
int amvpt_host_write_png(const char *path, const uint8_t *rgb, uint32_t width, uint32_t height);

/* Known-answer hooks (sensor.cpp / sensor.h). fov_axis: "x","y","smaller","larger","diagonal". */
double amvpt_host_parse_fov(double fov, const char *fov_axis, const char *focal_length, double aspect);
void amvpt_host_perspective_projection(const int *film_size, const int *crop_size,
                                       const int *crop_offset, float fov_x, float near_clip,
                                       float far_clip, float *matrix16);

#ifdef __cplusplus
}
#endif

#endif /* AMVPT_HOST_H */
