// projection_rays_host -- a stand-alone host program over octpt_projection_rays, for sanitizer runs of
// the host entry (tests/test_projection_cpu.py compiles it with octpt_host.cpp under -fsanitize=address,undefined).
// Reads cases from the file named by argv[1] and prints each case's rays:
//   in:  mode width height seed sample centre  eye[3] direction[3] up[3] fov param   (floats as C99 hex floats)
//   out: one line per case: the 6 * width * height ray words, then the width * height RNG states, as hex
// Every case is also run through the refusals, which must write nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/octpt.h"

static int fail(const char *what) {
    std::fprintf(stderr, "projection_rays_host: %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: projection_rays_host CASES");
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the cases file");
    unsigned mode, W, H, seed, sample, centre;
    while (std::fscanf(f, "%u %u %u %u %u %u", &mode, &W, &H, &seed, &sample, &centre) == 6) {
        float v[11];
        for (float &x : v)
            if (std::fscanf(f, "%f", &x) != 1) return fail("bad case row");
        octpt_camera cam{};
        std::memcpy(cam.eye, v, 12);
        std::memcpy(cam.direction, v + 3, 12);
        std::memcpy(cam.up, v + 6, 12);
        cam.fov = v[9];
        octpt_projection proj{};
        proj.mode = mode;
        proj.param = v[10];
        const size_t n = (size_t)W * H;
        // exact-size arrays: a read or write past any of them is the sanitizer's to report
        std::vector<uint32_t> xys(3 * n), state(n);
        std::vector<float> rays(6 * n);
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                uint32_t *r = &xys[3 * ((size_t)y * W + x)];
                r[0] = x;
                r[1] = y;
                r[2] = sample;
            }
        const uint32_t flags = centre ? OCTPT_PROJECTION_RAYS_CENTRE : 0u;
        // the refusals first, into marked arrays: nothing may be written
        const float mark = 123.25f;
        for (float &x : rays) x = mark;
        for (uint32_t &s : state) s = 0xA5A5A5A5u;
        for (int bad = 0; bad < 6; ++bad) {
            octpt_projection p = proj;
            octpt_camera c = cam;
            std::vector<uint32_t> q = xys;
            uint32_t fl = flags;
            octpt_status want = OCTPT_ERR_INVALID_ARG;
            if (bad == 0) p.mode = 7u, want = OCTPT_ERR_UNSUPPORTED;
            if (bad == 1) p.reserved[5] = 1u;
            if (bad == 2) p.mode = OCTPT_PROJECTION_FISHEYE, p.param = 7.0f;  // above 2 pi
            if (bad == 3) c.aperture = 0.5f, c.focal_distance = 2.0f, p.mode = OCTPT_PROJECTION_PARALLEL, p.param = 1.0f,
                          want = OCTPT_ERR_UNSUPPORTED;
            if (bad == 4) q[3 * (n - 1)] = W;  // the last row's pixel lies outside the frame
            if (bad == 5) fl |= 0x80u;
            if (octpt_projection_rays(&c, &p, W, H, seed, q.data(), (uint32_t)n, fl, rays.data(), state.data()) != want)
                return fail("a refusal returned another status");
        }
        for (float x : rays)
            if (x != mark) return fail("a refused call wrote rays");
        for (uint32_t s : state)
            if (s != 0xA5A5A5A5u) return fail("a refused call wrote states");
        if (octpt_projection_rays(&cam, &proj, W, H, seed, xys.data(), (uint32_t)n, flags, rays.data(), nullptr) != OCTPT_OK)
            return fail("the case was refused");
        std::vector<float> again(6 * n);
        if (octpt_projection_rays(&cam, &proj, W, H, seed, xys.data(), (uint32_t)n, flags, again.data(), state.data()) !=
            OCTPT_OK)
            return fail("the case was refused");
        if (std::memcmp(rays.data(), again.data(), rays.size() * sizeof(float)) != 0)
            return fail("the rays depend on the state pointer");
        for (float x : rays) {
            uint32_t u;
            std::memcpy(&u, &x, 4);
            std::printf("%x ", u);
        }
        for (uint32_t s : state) std::printf("%x ", s);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
