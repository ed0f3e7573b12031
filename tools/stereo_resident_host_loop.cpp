// Frame::ComputeStereoFromRGBD as a host loop over downloaded key points, for tools/stereo_resident_latency.py: the member's text per feature, every
// frame of a batch, one core.  Returns the mean time of `runs` passes over the batch in microseconds (std::chrono::steady_clock around the passes).
// Built by the tool with g++ -O2 -shared; nothing else uses it.
#include <chrono>
#include <cstddef>
#include <cstdint>

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };   // orbx_keypoint's layout

extern "C" double rgbd_host_loop(const KeyPoint *kps, const KeyPoint *kps_un, const int32_t *counts, int cap, int frames, const unsigned char *depth,
                                 size_t pitch, size_t frame_stride, float bf, float *u_right, float *out_depth, int runs) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < runs; r++)
        for (int f = 0; f < frames; f++) {
            const unsigned char *img = depth + (size_t)f * frame_stride;
            for (int i = 0; i < counts[f]; i++) {
                const size_t o = (size_t)f * cap + i;
                const float u = kps[o].x, v = kps[o].y;
                const float d = *reinterpret_cast<const float *>(img + (size_t)(int)v * pitch + 4 * (size_t)(int)u);
                if (d > 0) { out_depth[o] = d; u_right[o] = kps_un[o].x - bf / d; }
                else { out_depth[o] = -1.f; u_right[o] = -1.f; }
            }
        }
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / runs;
}
