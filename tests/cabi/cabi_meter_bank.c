/* A plain-C99 client of the meter banks of include/soundscope_hip.h: a bank of four stereo meters, two blocks of 10 ms, a
 * selective reset, one read.  Built and run by tests/test_meter_bank_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).
 * Prints one line of "key=value" pairs. */
#include <stdio.h>
#include <string.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 4, C = 2, FRAMES = 480 };
    static float pcm[N * FRAMES * C];
    ss_meter_bank *m = NULL;
    ss_meter_reading r[N];
    uint32_t one = 2u;
    unsigned i;
    int rc;
    for (i = 0; i < N * FRAMES * C; i++) pcm[i] = (float)((i % 97u) * 0.01 - 0.48);
    printf("abi=%d devices=%d sizeof_reading=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof r[0]);
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        if ((rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK && (rc = ss_meter_bank_reset(m, &one, 1u)) == SS_OK &&
            (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK && (rc = ss_meter_bank_read(m, r, N)) == SS_OK)
            printf(" m0=%.6f frames0=%llu frames2=%llu", r[0].momentary, (unsigned long long)r[0].frames,
                   (unsigned long long)r[2].frames);
        printf(" run=%d", rc);
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
