/* A plain-C99 client of the batch spectrogram of include/soundscope_hip.h: a two-stream pass, one view of it, both streams'
 * pictures in one download.  Built and run by tests/test_spectrogram_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one
 * line of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    ss_batch_config cfg;
    ss_batch_layout lay;
    ss_spectrogram_view view;
    ss_batch *b = NULL;
    uint32_t runs = 0u, run_windows = 0u, first = 0u, end = 0u;
    int rc;
    memset(&cfg, 0, sizeof cfg);
    memset(&lay, 0, sizeof lay);
    memset(&view, 0, sizeof view);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = 2; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_FFT; cfg.frames_per_stream = 48000;
    view.t_cols = 5u; view.f_cols = 16u; view.w_min = 0u; view.w_max = 42u; view.gain_mode = SS_GAIN_FIXED; view.gain_db = 0.0f;
    ss_spectrogram_column_windows(&view, 4u, &first, &end);
    printf("abi=%d devices=%d sizeof_view=%u last_first=%u last_end=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof view,
           (unsigned)first, (unsigned)end);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        float *cells = NULL;
        size_t n = 0, i, finite = 0;
        int early = ss_batch_download_spectrogram(b, 0u, 2u, NULL, 0u);
        if ((rc = ss_batch_layout_get(b, &lay)) == SS_OK) {
            n = (size_t)2 * lay.fft_channels * view.t_cols * view.f_cols;
            cells = (float *)malloc(n * sizeof *cells);
            if (!cells) rc = SS_ERR_NOMEM;
        }
        if (rc == SS_OK && (rc = ss_batch_synthesize(b, 7u, 0u)) == SS_OK && (rc = ss_batch_run(b)) == SS_OK &&
            (rc = ss_batch_spectrogram_plan(b, &view, &runs, &run_windows)) == SS_OK && (rc = ss_batch_spectrogram(b, &view)) == SS_OK &&
            (rc = ss_batch_download_spectrogram(b, 0u, 2u, cells, n)) == SS_OK) {
            for (i = 0; i < n; i++) finite += cells[i] >= -100.0f && cells[i] <= 0.0f;
            printf(" windows=%u cells=%lu in_chart=%lu runs=%u run_windows=%u short=%d", (unsigned)lay.n_windows, (unsigned long)n,
                   (unsigned long)finite, (unsigned)runs, (unsigned)run_windows, ss_batch_download_spectrogram(b, 0u, 2u, cells, n - 1u));
        }
        printf(" early=%d run=%d", early, rc);
        free(cells);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
