/* A plain-C99 client of the batch spectrum statistics of include/soundscope_hip.h: a two-stream pass, the reduction, stream 1's
 * average and peak-hold spectrum and the pooled batch's.  Built and run by tests/test_spectrum_stats_abi.py (CPU: must fail loudly
 * with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch_layout lay;
    ss_batch *b = NULL;
    uint32_t counted[2] = {0u, 0u}, chunks = 0u, chunk_windows = 0u;
    uint64_t pooled[2] = {0u, 0u};
    int rc;
    memset(&cfg, 0, sizeof cfg);
    memset(&lay, 0, sizeof lay);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 2; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_FFT; cfg.frames_per_stream = 48000;
    printf("abi=%d devices=%d ", ss_abi_version(), ss_device_count());
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        float *mean = NULL, *peak = NULL;
        size_t n = 0;
        int early = ss_batch_download_spectrum_stats(b, 0u, NULL, NULL, (size_t)-1, counted, 2u);
        if ((rc = ss_batch_layout_get(b, &lay)) == SS_OK) {
            n = (size_t)lay.fft_channels * lay.n_bins;
            mean = (float *)malloc(n * sizeof *mean);
            peak = (float *)malloc(n * sizeof *peak);
            if (!mean || !peak) rc = SS_ERR_NOMEM;
        }
        if (rc == SS_OK && (rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_run(b)) == SS_OK &&
            (rc = ss_batch_spectrum_stats_plan(b, &chunks, &chunk_windows)) == SS_OK && (rc = ss_batch_spectrum_stats(b)) == SS_OK &&
            (rc = ss_batch_download_spectrum_stats(b, 1u, mean, peak, n, counted, 2u)) == SS_OK) {
            printf(" windows=%u counted_mid=%u counted_side=%u mean0=%.4f max0=%.4f chunks=%u chunk_windows=%u", (unsigned)lay.n_windows,
                   (unsigned)counted[0], (unsigned)counted[1], (double)mean[0], (double)peak[0], (unsigned)chunks, (unsigned)chunk_windows);
            if ((rc = ss_batch_corpus_spectrum(b, mean, peak, n, pooled, 2u)) == SS_OK)
                printf(" pooled_mid=%lu pooled_side=%lu", (unsigned long)pooled[0], (unsigned long)pooled[1]);
        }
        printf(" early=%d run=%d", early, rc);
        free(mean);
        free(peak);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
