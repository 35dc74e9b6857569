/* A plain-C99 client of the batch resampler of include/soundscope_hip.h: the host functions first (they need no device) — the plan of
 * 32 -> 48 kHz, its table, the length rule and the reference chain over a stereo ramp — then four synthesised streams converted on
 * the device and stream 2 compared with the reference chain.  Built and run by tests/test_resample_abi.py (CPU: ss_batch_create
 * must fail loudly with SS_ERR_DEVICE, the host functions still answer).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

#define FRAMES 9001u
#define FRAMES_OUT 13502u   /* ceil(9001 * 3 / 2) */
#define N 40u

int main(void)
{
    ss_batch_config cfg;
    ss_batch *src = NULL, *dst = NULL;
    ss_resample_plan plan, other;
    ss_stream_shape shape;
    static float taps[3 * 72], x[N * 2], y[60 * 2], in[FRAMES * 2], out[FRAMES_OUT * 2], ref[FRAMES_OUT * 2];
    uint32_t tile_out = 0u, tile_in = 0u, i;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 32000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = FRAMES;
    printf("abi=%d devices=%d sizeof_plan=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof plan);
    rc = ss_resample_plan_make(32000u, 48000u, 0.0, 0.0, &plan);
    printf("make=%d make_equal=%d make_wide=%d up=%u down=%u taps=%u ", rc, ss_resample_plan_make(48000u, 48000u, 0.0, 0.0, &other),
           ss_resample_plan_make(44100u, 192000u, 0.0, 0.0, &other), (unsigned)plan.up, (unsigned)plan.down, (unsigned)plan.taps);
    printf("length=%llu table=%d ", (unsigned long long)ss_resample_length(&plan, N), ss_resample_taps(&plan, taps, sizeof taps / sizeof taps[0]));
    for (i = 0u; i < N; i++) { x[2u * i] = 0.25f * (float)i; x[2u * i + 1u] = -0.25f * (float)i; }
    printf("centre=%.9g host=%d y=", (double)taps[35], ss_resample_host(&plan, taps, x, N, 2u, 0u, 60u, y));
    for (i = 0u; i < 120u; i++) printf("%s%.9g", i ? "," : "", (double)y[i]);
    rc = ss_batch_create(&cfg, &src);
    printf(" create=%d", rc);
    if (rc == SS_OK) {
        cfg.sample_rate = 48000; cfg.frames_per_stream = FRAMES_OUT;
        if ((rc = ss_batch_create(&cfg, &dst)) == SS_OK && (rc = ss_batch_synthesize(src, 7u, 0u)) == SS_OK &&
            (rc = ss_batch_resample_plan(src, &plan, &tile_out, &tile_in)) == SS_OK && (rc = ss_batch_resample(src, dst, &plan)) == SS_OK &&
            (rc = ss_batch_stream_shape(dst, 2u, &shape)) == SS_OK && (rc = ss_batch_download_input(src, 2u, in, FRAMES * 2u)) == SS_OK &&
            (rc = ss_batch_download_input(dst, 2u, out, FRAMES_OUT * 2u)) == SS_OK &&
            (rc = ss_resample_host(&plan, taps, in, FRAMES, 2u, 0u, FRAMES_OUT, ref)) == SS_OK)
            printf(" tile_out=%u tile_in=%u frames=%llu passed=%d", (unsigned)tile_out, (unsigned)tile_in, (unsigned long long)shape.frames,
                   memcmp(out, ref, sizeof ref) == 0);
        printf(" run=%d", rc);
        if (dst) ss_batch_destroy(dst);
        ss_batch_destroy(src);
    }
    printf("\n");
    return 0;
}
