/* A plain-C99 client of the batch gain and the PCM export of include/soundscope_hip.h: the two host functions first (they need no
 * device), then a constant gain on stream 0 and a fade on stream 2 of what was synthesised, the records, and stream 0 as 16-bit PCM.
 * Built and run by tests/test_apply_gain_abi.py (CPU: ss_batch_create must fail loudly with SS_ERR_DEVICE, the host functions
 * still answer).  Prints one line of "key=value" pairs. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

#define FRAMES 9001u

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_normalise_target target;
    ss_gain_point pts[3];
    ss_gain_config gcfg;
    ss_pcm_dither dither;
    static ss_gain_channel stats[4 * 2];
    static short pcm[FRAMES * 2u];
    double gain_db = 0.0;
    float gain = 0.0f;
    uint32_t why = 0u, tile = 0u;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = FRAMES;
    target.target_lufs = -23.0; target.max_true_peak_dbtp = -1.0; target.max_gain_db = INFINITY; target.min_gain_db = -INFINITY;
    pts[0].frame = 0u; pts[0].stream = 0u; pts[0].gain = 0.5f;
    pts[1].frame = 100u; pts[1].stream = 2u; pts[1].gain = 1.0f;
    pts[2].frame = 108u; pts[2].stream = 2u; pts[2].gain = 0.0f;
    gcfg.channel_mask = 0u; gcfg.clip_level = 1.0f; gcfg.reserved = 0u;
    dither.seed = 1u; dither.kind = SS_DITHER_TPDF; dither.reserved = 0u;
    printf("abi=%d devices=%d sizeof_target=%u sizeof_point=%u sizeof_config=%u sizeof_channel=%u sizeof_dither=%u ", ss_abi_version(),
           ss_device_count(), (unsigned)sizeof target, (unsigned)sizeof pts[0], (unsigned)sizeof gcfg, (unsigned)sizeof stats[0],
           (unsigned)sizeof dither);
    rc = ss_normalisation_gain(&target, -20.0, 0.5, &gain_db, &gain, &why);
    printf("law=%d gain_db=%.17g gain=%.9g limited_by=%u ", rc, gain_db, (double)gain, (unsigned)why);
    target.min_gain_db = NAN;
    printf("law_nan=%d ", ss_normalisation_gain(&target, -20.0, 0.5, NULL, NULL, NULL));
    printf("env_mid=%.17g env_before=%.17g env_behind=%.17g ", ss_gain_envelope(pts + 1, 2u, 102u), ss_gain_envelope(pts + 1, 2u, 0u),
           ss_gain_envelope(pts + 1, 2u, 5000u));
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_apply_gain_plan(b, &tile)) == SS_OK &&
            (rc = ss_batch_apply_gain(b, pts, 3u, &gcfg)) == SS_OK && (rc = ss_batch_download_gain_stats(b, stats, 8u)) == SS_OK &&
            (rc = ss_batch_download_pcm(b, 0u, 1u, pcm, sizeof pcm, SS_PCM_S16, &dither)) == SS_OK)
            printf(" tile=%u touched=%u%u%u%u peak_ok=%d", (unsigned)tile, (unsigned)stats[0].touched, (unsigned)stats[2].touched,
                   (unsigned)stats[4].touched, (unsigned)stats[6].touched, stats[0].sample_peak > 0.0f);
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
