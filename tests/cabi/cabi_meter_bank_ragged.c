/* A plain-C99 client of the ragged meter-bank adds of include/soundscope_hip.h: a bank of three stereo meters, two ragged calls
 * (the second with a stream that gets nothing, its pointer NULL), one read.  Built and run by tests/test_meter_bank_ragged_abi.py
 * (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 3, C = 2, LONGEST = 1000 };
    static float pcm[N][LONGEST * C];
    const float *blocks[N];
    const uint64_t first[N] = {480u, 1000u, 17u}, second[N] = {960u, 0u, 481u};
    ss_meter_bank *m = NULL;
    ss_meter_reading r[N];
    unsigned s, i;
    int rc;
    for (s = 0; s < N; s++)
        for (i = 0; i < LONGEST * C; i++) pcm[s][i] = (float)(((i + 31u * s) % 97u) * 0.01 - 0.48);
    printf("abi=%d devices=%d ", ss_abi_version(), ss_device_count());
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        for (s = 0; s < N; s++) blocks[s] = pcm[s];
        rc = ss_meter_bank_add_ragged(m, blocks, first);
        blocks[1] = NULL;
        if (rc == SS_OK && (rc = ss_meter_bank_add_ragged(m, blocks, second)) == SS_OK && (rc = ss_meter_bank_read(m, r, N)) == SS_OK)
            printf(" frames0=%llu frames1=%llu frames2=%llu", (unsigned long long)r[0].frames, (unsigned long long)r[1].frames,
                   (unsigned long long)r[2].frames);
        printf(" run=%d", rc);
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
