// tracker_fail_probe.cpp — stand-alone host program: walks the failure exits of the tracker host (sg_slam_amd/csrc/sgx_tracker.cpp) with sgx_tracker_debug_fail_after, which
// makes the n-th acquisition or checked call of a tracker entry fail.  tests/test_tracker_fail_probe.py builds this file and the emulator units with AddressSanitizer /
// UBSan; in the emulator hipMalloc is calloc and device pointers are host pointers, so LeakSanitizer sees what a failed call leaves behind, and ASan a later call that
// reads a half-built tracker.  One line per sweep; the first violation ends the program.
#include "../../include/sgx.h"
#include "../../include/sgx_debug.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

enum { W = 640, H = 480, S = 2 };
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "tracker_fail_probe: %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static sgx_tracker_config config(int pipelined, int dynamic_mask)
{
    sgx_tracker_config c; memset(&c, 0, sizeof c);
    c.streams = S; c.width = W; c.height = H; c.nfeatures = 1000; c.scale_factor = 1.2f; c.nlevels = 8; c.ini_th_fast = 20; c.min_th_fast = 7;
    c.cam.fx = 535.4f; c.cam.fy = 539.2f; c.cam.cx = 320.1f; c.cam.cy = 247.6f; c.cam.bf = 40.0f; c.cam.max_x = W; c.cam.max_y = H;
    c.depth_map_factor = 5000.0f; c.th_projection = 15.0f; c.local_map = 1; c.dynamic_mask = dynamic_mask; c.max_boxes = 8; c.pipelined = pipelined;
    return c;
}

// frames: a gradient with a few bright squares that move one pixel per frame (a handful of corners: only the host paths are under test), constant depth of one metre
struct Frames {
    std::vector<uint8_t> gray, bgr; std::vector<uint16_t> depth;
    explicit Frames(int t) : gray((size_t)S * H * W), bgr((size_t)S * H * W * 3), depth((size_t)S * H * W, 5000)
    {
        for (int s = 0; s < S; s++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            const int u = x - t - 7 * s, v = y - t;
            const bool square = u > 40 && v > 40 && u % 80 < 24 && v % 80 < 24;
            const uint8_t g = square ? 230 : (uint8_t)(40 + (x + y) / 16);
            const size_t k = ((size_t)s * H + y) * W + x;
            gray[k] = g; bgr[3 * k] = bgr[3 * k + 1] = bgr[3 * k + 2] = g;
        }
    }
};

static sgx_tracker *create(int pipelined, int dynamic_mask)
{
    const sgx_tracker_config c = config(pipelined, dynamic_mask);
    sgx_tracker *t = nullptr;
    REQUIRE(sgx_tracker_create(&c, nullptr, &t) == SGX_OK && t, "create(pipelined %d, mask %d) failed", pipelined, dynamic_mask);
    return t;
}
static int step(sgx_tracker *t, int frame) { const Frames f(frame); return sgx_tracker_step_dev(t, f.gray.data(), W, f.depth.data(), nullptr, 0, nullptr); }      // the emulator reads the frames inside the call

struct Read { float Tcw[S * 16]; int32_t v[7][S], f_stats[S * 4]; };
static Read read(sgx_tracker *t)
{
    Read r; memset(&r, 0, sizeof r);
    REQUIRE(sgx_tracker_read(t, r.Tcw, r.v[0], r.v[1], r.v[2], r.v[3], r.v[4], r.v[5], r.v[6], r.f_stats) == SGX_OK, "read failed");
    return r;
}

// arms the injection, runs `call`, disarms: the call's status, and whether it is the status that was injected (a call the injection did not reach must succeed)
template <class F> static int injected(int n, F call, bool *fired)
{
    sgx_tracker_debug_fail_after(n);
    const int rc = call();
    const int delivered = sgx_tracker_debug_fail_after(0);
    *fired = delivered != SGX_OK;
    REQUIRE(rc == delivered, "n = %d: the call returned %d, the injected failure was %d", n, rc, delivered);
    REQUIRE(rc == SGX_OK || rc == SGX_ERR_NOMEM || rc == SGX_ERR_DEVICE, "n = %d: status %d", n, rc);
    return rc;
}

static void sweep_create()
{
    for (int pipelined = 0; pipelined < 2; pipelined++) for (int mask = 0; mask < 2; mask++) {
        const sgx_tracker_config c = config(pipelined, mask);
        int nomem = 0, device = 0, n = 1;
        for (;; n++) {
            sgx_tracker *t = (sgx_tracker *)&c;        // anything but NULL: a failed create must clear it
            bool fired;
            const int rc = injected(n, [&] { return sgx_tracker_create(&c, nullptr, &t); }, &fired);
            REQUIRE((rc == SGX_OK) == (t != nullptr), "create n = %d: status %d with handle %s", n, rc, t ? "set" : "NULL");
            if (rc == SGX_OK) { sgx_tracker_destroy(t); break; }
            (rc == SGX_ERR_NOMEM ? nomem : device)++;
        }
        REQUIRE(nomem > 0 && device > 0 && nomem + device == n - 1, "create: %d + %d failures of %d", nomem, device, n - 1);
        printf("create pipelined %d mask %d: succeeds at n = %d (%d acquisitions: %d allocations refused with NOMEM, %d other calls with DEVICE)\n", pipelined, mask, n, n - 1, nomem, device);
    }
    sgx_tracker_config bad = config(1, 1); bad.streams = 0;
    sgx_tracker *t = (sgx_tracker *)&bad;
    REQUIRE(sgx_tracker_create(&bad, nullptr, &t) == SGX_ERR_INVALID && !t, "streams 0: not refused as invalid with a NULL handle");
}

static void fill(uint8_t *bgr, int pitch, uint16_t *depth, const Frames &f)
{
    for (int r = 0; r < S * H; r++) memcpy(bgr + (size_t)r * pitch, f.bgr.data() + (size_t)r * W * 3, (size_t)W * 3);
    memcpy(depth, f.depth.data(), f.depth.size() * 2);
}

static void sweep_host_buffers()
{
    for (int pipelined = 0; pipelined < 2; pipelined++) {
        const Frames f(0);
        uint8_t *b = nullptr; uint16_t *d = nullptr; int pitch = 0;
        sgx_tracker *ref = create(pipelined, 1);
        REQUIRE(sgx_tracker_host_buffers(ref, 0, &b, &pitch, &d) == SGX_OK, "host_buffers failed");
        fill(b, pitch, d, f);
        REQUIRE(sgx_tracker_step_host(ref, 0, 1) == SGX_OK, "step_host failed");
        const Read expected = read(ref);
        sgx_tracker_destroy(ref);
        int n = 1;
        for (;; n++) {
            sgx_tracker *t = create(pipelined, 1);
            bool fired;
            b = nullptr; d = nullptr;
            const int rc = injected(n, [&] { return sgx_tracker_host_buffers(t, 0, &b, &pitch, &d); }, &fired);
            if (rc != SGX_OK) {
                REQUIRE(sgx_tracker_step_host(t, 0, 1) == SGX_ERR_INVALID, "host_buffers n = %d: the failed call left staging behind", n);
                b = nullptr; d = nullptr;
                REQUIRE(sgx_tracker_host_buffers(t, 0, &b, &pitch, &d) == SGX_OK && b && d && pitch >= 3 * W, "host_buffers n = %d: the retry failed", n);
                uint8_t *b1 = nullptr; uint16_t *d1 = nullptr;
                REQUIRE(sgx_tracker_host_buffers(t, 1, &b1, nullptr, &d1) == SGX_OK && b1 && d1 && b1 != b, "host_buffers n = %d: slot 1 after the retry", n);
                fill(b, pitch, d, f);
                REQUIRE(sgx_tracker_step_host(t, 0, 1) == SGX_OK, "host_buffers n = %d: step_host after the retry failed", n);
                const Read got = read(t);
                REQUIRE(memcmp(&got, &expected, sizeof got) == 0, "host_buffers n = %d: results differ from a tracker that never saw a failure", n);
            }
            sgx_tracker_destroy(t);
            if (rc == SGX_OK) break;
        }
        REQUIRE(n > 1, "host_buffers: the injection reached nothing");
        printf("host_buffers pipelined %d: %d failing calls, each retried, stepped and equal to the undisturbed tracker\n", pipelined, n - 1);
    }
}

static void sweep_set_distortion()
{
    const float dist[5] = { 0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f };      // TUM1.yaml
    int n = 1;
    for (;; n++) {
        int rc = SGX_OK;
        for (int retry = 0; retry < 2; retry++) {
            sgx_tracker *t = create(1, 0);
            bool fired;
            rc = injected(n, [&] { return sgx_tracker_set_distortion(t, dist, 5, nullptr); }, &fired);
            const bool undistorting = rc == SGX_OK || retry;
            if (rc != SGX_OK && retry) REQUIRE(sgx_tracker_set_distortion(t, dist, 5, nullptr) == SGX_OK, "set_distortion n = %d: the retry failed", n);
            REQUIRE(step(t, 0) == SGX_OK, "set_distortion n = %d: step failed", n);
            const sgx_keypoint *keys = nullptr, *keys_un = nullptr;
            REQUIRE(sgx_tracker_frame_dev(t, nullptr, &keys, nullptr, nullptr, nullptr, nullptr) == SGX_OK && sgx_tracker_frame_keys_un_dev(t, &keys_un) == SGX_OK && keys && keys_un, "frame_dev");
            REQUIRE((keys_un != keys) == undistorting, "set_distortion n = %d: %s keys after %s", n, keys_un != keys ? "undistorted" : "distorted", undistorting ? "a successful call" : "a failed call");
            REQUIRE(sgx_tracker_sync(t) == SGX_OK, "sync");
            sgx_tracker_destroy(t);
            if (rc == SGX_OK) break;
        }
        if (rc == SGX_OK) break;
    }
    REQUIRE(n > 1, "set_distortion: the injection reached nothing");
    printf("set_distortion: %d failing calls; distorted keys after each, undistorted keys after each retry\n", n - 1);
}

static void sweep_step()
{
    std::vector<uint8_t> rec;
    int n = 1;
    for (;; n++) {
        sgx_tracker *t = create(1, 1);
        REQUIRE(step(t, 0) == SGX_OK, "first step failed");
        bool fired;
        const int rc = injected(n, [&] { return step(t, 1); }, &fired);
        if (rc != SGX_OK) {
            rec.resize((size_t)S * sgx_tracker_record_bytes(t) + 4);
            REQUIRE(step(t, 2) == rc && step(t, 3) == rc, "step n = %d: the steps after the failed one do not return its status %d", n, rc);
            REQUIRE(sgx_tracker_pack_records_dev(t, rec.data(), nullptr) == rc, "step n = %d: pack_records on a poisoned tracker", n);
            REQUIRE(sgx_tracker_wait_inputs(t, 0) == SGX_OK && sgx_tracker_sync(t) == SGX_OK, "step n = %d: wait_inputs / sync on a poisoned tracker", n);
            (void)read(t);
        }
        sgx_tracker_destroy(t);
        if (rc == SGX_OK) break;
    }
    REQUIRE(n > 1, "step: the injection reached nothing");
    printf("step: %d failing second steps, each poisons the tracker; sync, read and destroy go on working\n", n - 1);
    {   // a failure on the host-input path poisons as well
        sgx_tracker *t = create(1, 1);
        uint8_t *b = nullptr; uint16_t *d = nullptr; int pitch = 0; bool fired;
        REQUIRE(sgx_tracker_host_buffers(t, 0, &b, &pitch, &d) == SGX_OK, "host_buffers failed");
        fill(b, pitch, d, Frames(0));
        const int rc = injected(1, [&] { return sgx_tracker_step_host(t, 0, 1); }, &fired);
        REQUIRE(rc == SGX_ERR_DEVICE && sgx_tracker_step_host(t, 0, 1) == rc && step(t, 1) == rc && sgx_tracker_sync(t) == SGX_OK, "step_host: a failed upload does not poison");
        sgx_tracker_destroy(t);
    }
    {   // an argument refusal is not a failed step
        sgx_tracker *t = create(1, 1);
        const Frames f(0);
        REQUIRE(sgx_tracker_step_dev(t, f.gray.data(), W - 1, f.depth.data(), nullptr, 0, nullptr) == SGX_ERR_INVALID, "gray_pitch < width not refused");
        REQUIRE(step(t, 0) == SGX_OK && step(t, 1) == SGX_OK, "the step after a refused one failed");
        (void)read(t);
        sgx_tracker_destroy(t);
        printf("step: gray_pitch < width is refused and poisons nothing\n");
    }
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);          // a sanitizer report ends the program without flushing
    sweep_create();
    sweep_host_buffers();
    sweep_set_distortion();
    sweep_step();
    printf("tracker_fail_probe: ok\n");
    return 0;
}
