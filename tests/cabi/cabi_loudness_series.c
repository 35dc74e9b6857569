/* A plain-C99 client of the loudness series of include/soundscope_hip.h: a batch made with SS_BATCH_LOUDNESS_SERIES, one pass,
 * the series of stream 0 and every stream's maxima.  Built and run by tests/test_loudness_series_abi.py (CPU: must fail loudly
 * with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch *b = NULL;
    ss_loudness_extremes ext[4];
    double m[30], s[30];
    int rc;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 4; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_LUFS | SS_BATCH_LOUDNESS_SERIES; cfg.frames_per_stream = 48000 * 3;
    printf("abi=%d devices=%d sizeof_extremes=%u flag=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof ext[0],
           (unsigned)SS_BATCH_LOUDNESS_SERIES);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_run(b)) == SS_OK &&
            (rc = ss_batch_download_loudness_series(b, 0u, m, s, 30u)) == SS_OK && (rc = ss_batch_loudness_extremes(b, ext, 4u)) == SS_OK)
            printf(" m29=%.6f s29=%.6f max_m=%.6f at_m=%u max_s=%.6f at_s=%u", m[29], s[29], ext[0].max_momentary,
                   (unsigned)ext[0].max_momentary_at, ext[0].max_shortterm, (unsigned)ext[0].max_shortterm_at);
        printf(" run=%d", rc);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
