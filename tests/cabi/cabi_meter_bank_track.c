/* A plain-C99 client of the tracked meter-bank spectra of include/soundscope_hip.h: a bank of two stereo meters with the spectrum
 * and its tracking on, two blocks of 10 ms with an update behind each, the two curves as rows and as 160 columns.  Built and run
 * by tests/test_meter_bank_track_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 2, C = 2, FRAMES = 480, COLS = 160 };
    static float pcm[N * FRAMES * C];
    static float acols[N * 2 * COLS], hcols[N * 2 * COLS];
    const ss_spectrum_ballistics cfg = {0.125, 0.5, 16.0};
    ss_meter_bank *m = NULL;
    uint32_t rows = 0, bins = 0, updates[N * 2] = {0, 0, 0, 0};
    float *avg = NULL, *hold = NULL;
    unsigned i;
    int rc;
    for (i = 0; i < N * FRAMES * C; i++) pcm[i] = (float)((i % 89u) * 0.01 - 0.44);
    printf("abi=%d devices=%d sizeof_cfg=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof(ss_spectrum_ballistics));
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        printf(" no_history=%d", ss_meter_bank_spectrum_track_enable(m, &cfg));
        rc = ss_meter_bank_spectrum_enable(m, 1);
        printf(" before=%d", ss_meter_bank_spectrum_track(m));
        if (rc == SS_OK && (rc = ss_meter_bank_spectrum_track_enable(m, &cfg)) == SS_OK &&
            (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK && (rc = ss_meter_bank_spectrum_track(m)) == SS_OK &&
            (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK && (rc = ss_meter_bank_spectrum_track(m)) == SS_OK &&
            (rc = ss_meter_bank_spectrum_layout(m, &rows, &bins, NULL, NULL, 0)) == SS_OK) {
            avg = (float *)malloc(sizeof(float) * N * rows * bins);
            hold = (float *)malloc(sizeof(float) * N * rows * bins);
            if (avg && hold && (rc = ss_meter_bank_spectrum_tracked(m, avg, hold, (size_t)N * rows * bins, updates, N * rows)) == SS_OK &&
                (rc = ss_meter_bank_spectrum_tracked_columns(m, COLS, SS_GAIN_REFERENCE, 0.0f, acols, hcols, (size_t)N * rows * COLS,
                                                             NULL, 0)) == SS_OK)
                printf(" rows=%u bins=%u updates0=%u updates3=%u hold_ge_avg=%d", rows, bins, updates[0], updates[3],
                       hold[100] >= avg[100] - 1e-3f);
            if (rc == SS_OK && (rc = ss_meter_bank_spectrum_track_reset(m, NULL, 0)) == SS_OK &&
                (rc = ss_meter_bank_spectrum_tracked(m, NULL, NULL, 0, updates, N * rows)) == SS_OK)
                printf(" after_reset=%u", updates[0]);
            free(avg);
            free(hold);
        }
        printf(" run=%d off=%d", rc, ss_meter_bank_spectrum_track_enable(m, NULL));
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
