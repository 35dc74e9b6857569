/* A plain-C99 client of the meter-bank spectra of include/soundscope_hip.h: a bank of two stereo meters with the spectrum on,
 * one block of 10 ms, the layout, the rows and 160 columns at the reference gain.  Built and run by
 * tests/test_meter_bank_spectrum_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 2, C = 2, FRAMES = 480, COLS = 160 };
    static float pcm[N * FRAMES * C];
    ss_meter_bank *m = NULL;
    uint32_t rows = 0, bins = 0;
    int32_t status[N * 2];
    float *spec = NULL, *cols = NULL;
    unsigned i;
    int rc;
    for (i = 0; i < N * FRAMES * C; i++) pcm[i] = (float)((i % 89u) * 0.01 - 0.44);
    printf("abi=%d devices=%d window=%d ", ss_abi_version(), ss_device_count(), SS_BANK_SPECTRUM_N);
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        printf(" before=%d", ss_meter_bank_spectrum_layout(m, &rows, &bins, NULL, NULL, 0));
        if ((rc = ss_meter_bank_spectrum_enable(m, 1)) == SS_OK && (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK &&
            (rc = ss_meter_bank_spectrum_layout(m, &rows, &bins, NULL, NULL, 0)) == SS_OK) {
            spec = (float *)malloc(sizeof(float) * N * rows * bins);
            cols = (float *)malloc(sizeof(float) * N * rows * COLS);
            if (spec && cols && (rc = ss_meter_bank_spectrum(m, spec, (size_t)N * rows * bins, status, N * rows)) == SS_OK &&
                (rc = ss_meter_bank_spectrum_columns(m, COLS, SS_GAIN_REFERENCE, 0.0f, cols, (size_t)N * rows * COLS, status,
                                                     N * rows)) == SS_OK)
                printf(" rows=%u bins=%u status0=%d", rows, bins, status[0]);
            free(spec);
            free(cols);
        }
        printf(" run=%d", rc);
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
