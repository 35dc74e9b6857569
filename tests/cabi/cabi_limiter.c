/* A plain-C99 client of the batch limiter of include/soundscope_hip.h: the host function first (it needs no device), then streams
 * 0 and 2 of what was synthesised limited under a low ceiling, and the records.  Built and run by tests/test_limiter_abi.py (CPU:
 * ss_batch_create must fail loudly with SS_ERR_DEVICE, the host function still answers).  Prints one line of "key=value" pairs. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

#define FRAMES 9001u
#define N 12u

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_limit_config lcfg;
    ss_limit_item items[2];
    static ss_limit_stream streams[4];
    static ss_gain_channel stats[4 * 2];
    float level[N];
    uint32_t r_q[N], tile = 0u, group = 0u, i;
    uint64_t sum[N], scratch = 0u;
    double curve[N];
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = FRAMES;
    memset(&lcfg, 0, sizeof lcfg);
    lcfg.channel_mask = 0u; lcfg.ceiling = 0.5f; lcfg.clip_level = 1.0f; lcfg.lookahead = 2u; lcfg.hold = 1u;
    lcfg.detector = SS_LIMIT_SAMPLE_PEAK; lcfg.reserved = 0u; lcfg.scratch_bytes = 0u;
    items[0].stream = 2u; items[0].gain = -1.5f;
    items[1].stream = 0u; items[1].gain = 1.0f;
    for (i = 0u; i < N; i++) level[i] = 0.1f;
    level[6] = 0.9f;
    printf("abi=%d devices=%d sizeof_item=%u sizeof_config=%u sizeof_stream=%u ", ss_abi_version(), ss_device_count(),
           (unsigned)sizeof items[0], (unsigned)sizeof lcfg, (unsigned)sizeof streams[0]);
    rc = ss_limit_curve(level, N, 1.0f, &lcfg, 0u, r_q, sum, curve);
    printf("curve=%d r_q=", rc);
    for (i = 0u; i < N; i++) printf("%s%lu", i ? "," : "", (unsigned long)r_q[i]);
    printf(" sum=");
    for (i = 0u; i < N; i++) printf("%s%llu", i ? "," : "", (unsigned long long)sum[i]);
    printf(" c=");
    for (i = 0u; i < N; i++) printf("%s%.17g", i ? "," : "", curve[i]);
    printf(" curve_nan=%d ", ss_limit_curve(level, N, NAN, &lcfg, 0u, NULL, NULL, NULL));
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        lcfg.ceiling = 0.05f; lcfg.lookahead = 72u; lcfg.hold = 480u; lcfg.detector = SS_LIMIT_TRUE_PEAK;
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_limit_plan(b, &lcfg, 2u, &tile, &group, &scratch)) == SS_OK &&
            (rc = ss_batch_limit(b, items, 2u, &lcfg)) == SS_OK && (rc = ss_batch_download_limit_stats(b, streams, 4u, stats, 8u)) == SS_OK)
            printf(" tile=%u group=%u scratch=%llu touched=%u%u%u%u under=%d", (unsigned)tile, (unsigned)group, (unsigned long long)scratch,
                   (unsigned)streams[0].touched, (unsigned)streams[1].touched, (unsigned)streams[2].touched, (unsigned)streams[3].touched,
                   stats[0].sample_peak <= 0.05f && stats[1].sample_peak <= 0.05f && stats[4].sample_peak <= 0.05f && stats[5].sample_peak <= 0.05f);
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
