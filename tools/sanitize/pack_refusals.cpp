// Stand-alone host program: svr_pack_frames() called with every argument set it must refuse, and svr_last_error() read after each.
// For a sanitizer run of the entry point's host code on a machine without a GPU -- nothing here is ever launched:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         comfyui-seedvr2_videoupscaler_amd/csrc/svr_api.hip tools/sanitize/pack_refusals.cpp -o pack_refusals && ./pack_refusals
// Exit status 0: every call was refused with a message naming svr_pack_frames and the argument; the sanitizers report on stderr.
#include "../../include/seedvr2_hip.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

struct Case {
    const char* what; const char* word;
    int null_frames, null_out, kind, T, H, W, C, fmt;
    int64_t bytes_off;                     // added to the exact size of the format
    int frames_off, out_off;               // bytes added to the 16-byte aligned buffers
};

static int64_t exact(const Case& c) {                     // (unsigned: the huge case may wrap here, it is refused before the size counts)
    const uint64_t T = (uint64_t)c.T, H = (uint64_t)c.H, W = (uint64_t)c.W, h2 = (H + 1) / 2, w2 = (W + 1) / 2;
    return (int64_t)(c.fmt == SVR_PACK_YUV420P10 ? 2 * T * (H * W + 2 * h2 * w2) : T * H * W * (uint64_t)c.C);
}

int main() {
    alignas(16) static char frames[4096], out[4096];
    const Case cases[] = {
        {"null frames", "frames", 1, 0, SVR_STORE_FP32, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 0, 0},
        {"null out", "out", 0, 1, SVR_STORE_FP32, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 0, 0},
        {"h16 input", "x_kind", 0, 0, SVR_STORE_H16, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 0, 0},
        {"negative kind", "x_kind", 0, 0, -1, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 0, 0},
        {"T = 0", "T >= 1", 0, 0, SVR_STORE_FP32, 0, 4, 6, 3, SVR_PACK_RGB8, 0, 0, 0},
        {"H = 0", "H >= 1", 0, 0, SVR_STORE_BF16, 1, 0, 6, 3, SVR_PACK_BGR8, 0, 0, 0},
        {"W < 0", "W >= 1", 0, 0, SVR_STORE_BF16, 1, 4, -6, 3, SVR_PACK_YUV420P10, 0, 0, 0},
        {"unknown format", "fmt", 0, 0, SVR_STORE_FP32, 1, 4, 6, 3, 3, 0, 0, 0},
        {"negative format", "fmt", 0, 0, SVR_STORE_FP32, 1, 4, 6, 3, -2, 0, 0, 0},
        {"C = 2", "C must be", 0, 0, SVR_STORE_FP32, 1, 4, 6, 2, SVR_PACK_RGB8, 0, 0, 0},
        {"C = 5", "C must be", 0, 0, SVR_STORE_FP32, 1, 4, 6, 5, SVR_PACK_BGR8, 0, 0, 0},
        {"C = 4 for yuv420p10", "C must be 3", 0, 0, SVR_STORE_FP32, 1, 4, 6, 4, SVR_PACK_YUV420P10, 0, 0, 0},
        {"out_bytes one short", "out_bytes", 0, 0, SVR_STORE_FP32, 1, 4, 6, 3, SVR_PACK_RGB8, -1, 0, 0},
        {"out_bytes one long", "out_bytes", 0, 0, SVR_STORE_FP32, 2, 5, 7, 4, SVR_PACK_BGR8, 1, 0, 0},
        {"out_bytes of the even-size plane", "out_bytes", 0, 0, SVR_STORE_BF16, 2, 5, 7, 3, SVR_PACK_YUV420P10, -2 * 2 * (2 * 12 - 17), 0, 0},
        {"a clip beyond 2^40 pixels", "T * H * W", 0, 0, SVR_STORE_FP32, 2147483647, 2147483647, 2147483647, 3, SVR_PACK_YUV420P10, 8, 0, 0},
        {"misaligned fp32 frames", "frames", 0, 0, SVR_STORE_FP32, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 2, 0},
        {"misaligned bf16 frames", "frames", 0, 0, SVR_STORE_BF16, 1, 4, 6, 3, SVR_PACK_RGB8, 0, 1, 0},
        {"misaligned uint16 out", "out", 0, 0, SVR_STORE_FP32, 1, 4, 6, 3, SVR_PACK_YUV420P10, 0, 0, 1},
    };
    int bad = 0;
    for (const Case& c : cases) {
        const int rc = svr_pack_frames(c.null_frames ? nullptr : frames + c.frames_off, c.kind, c.T, c.H, c.W, c.C, c.fmt,
                                       c.null_out ? nullptr : out + c.out_off, exact(c) + c.bytes_off, nullptr);
        const char* msg = svr_last_error();
        const bool ok = rc != 0 && msg && strstr(msg, "svr_pack_frames") && strstr(msg, c.word);
        printf("%-34s rc %d  %s%s\n", c.what, rc, msg ? msg : "(no message)", ok ? "" : "    <-- NOT REFUSED AS EXPECTED");
        bad += !ok;
    }
    printf("%d of %zu calls refused as expected\n", (int)(sizeof(cases) / sizeof(cases[0])) - bad, sizeof(cases) / sizeof(cases[0]));
    return bad != 0;
}
