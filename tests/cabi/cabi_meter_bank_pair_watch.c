/* A plain-C99 client of the meter banks' pair watch of include/soundscope_hip.h: a bank of two stereo meters with the watch on, fed
 * two entries (200 ms) in three calls — stream 0's right channel is its left inverted (b = -a), stream 1's channels are equal — the
 * records and the ring after them, a selective reset, the watch off.  Built and run by tests/test_meter_bank_pair_watch_abi.py (CPU:
 * must fail loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <math.h>
#include <stdio.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 2, C = 2, S = 4800, CALLS = 3, FRAMES = 2 * S / CALLS };
    static float pcm[N * FRAMES * C];
    const ss_pair_watch_config cfg = {0.0, 0.0, 1u, 30u};
    ss_pair_watch_config wide = {0.0, 0.0, 1u, SS_BANK_PAIR_WINDOW_MAX + 1u};
    const ss_channel_pair bad = {0u, 2u};
    ss_pair_watch rec[N];
    ss_pair_entry ring[30];
    const uint32_t one = 1u;
    ss_meter_bank *m = NULL;
    uint32_t lanes = 0, window = 0, pairs = 0, n_entries = 0;
    uint64_t first = 7;
    unsigned i, call;
    int rc;
    for (i = 0; i < FRAMES; i++) {
        const float x = (float)(i % 7u) * 0.125f - 0.375f;
        pcm[i * C] = x; pcm[i * C + 1] = -x;
        pcm[(FRAMES + i) * C] = x; pcm[(FRAMES + i) * C + 1] = x;
    }
    printf("abi=%d devices=%d sizeof_sums=%u sizeof_config=%u sizeof_watch=%u sizeof_entry=%u ", ss_abi_version(), ss_device_count(),
           (unsigned)sizeof(ss_pair_sums), (unsigned)sizeof(ss_pair_watch_config), (unsigned)sizeof(ss_pair_watch), (unsigned)sizeof(ss_pair_entry));
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        printf(" before=%d", ss_meter_bank_pair_watch(m, rec, N));
        printf(" wide=%d badpair=%d", ss_meter_bank_pair_watch_enable(m, NULL, 0, &wide), ss_meter_bank_pair_watch_enable(m, &bad, 1, &cfg));
        rc = ss_meter_bank_pair_watch_enable(m, NULL, 0, &cfg);
        if (rc == SS_OK) rc = ss_meter_bank_pair_watch_plan(m, &lanes, &window, &pairs);
        for (call = 0; rc == SS_OK && call < CALLS; call++) rc = ss_meter_bank_add(m, pcm, FRAMES);
        if (rc == SS_OK && (rc = ss_meter_bank_pair_watch(m, rec, N)) == SS_OK &&
            (rc = ss_meter_bank_pair_watch_entries(m, 0, ring, 30, &first, &n_entries)) == SS_OK)
            printf(" lanes=%u window=%u pairs=%u entries=%lu open=%u n_below=%lu trailing=%lu first_below=%lu corr=%.17g same_below=%lu same_corr=%.17g"
                   " ring=%u first=%lu ring_frames=%u small=%d",
                   lanes, window, pairs, (unsigned long)rec[0].entries, rec[0].open_frames, (unsigned long)rec[0].n_below,
                   (unsigned long)rec[0].trailing_below, (unsigned long)rec[0].first_below,
                   rec[0].window.s_ab / sqrt(rec[0].window.s_aa * rec[0].window.s_bb), (unsigned long)rec[1].n_below,
                   rec[1].total.s_ab / sqrt(rec[1].total.s_aa * rec[1].total.s_bb), n_entries, (unsigned long)first, ring[1].frames,
                   ss_meter_bank_pair_watch(m, rec, N - 1));
        if (rc == SS_OK && (rc = ss_meter_bank_pair_watch_reset(m, &one, 1)) == SS_OK && (rc = ss_meter_bank_pair_watch(m, rec, N)) == SS_OK)
            printf(" kept=%lu after_reset=%lu", (unsigned long)rec[0].entries, (unsigned long)rec[1].entries);
        printf(" run=%d off=%d", rc, ss_meter_bank_pair_watch_enable(m, NULL, 0, NULL));
        printf(" after=%d", ss_meter_bank_pair_watch_plan(m, &lanes, &window, &pairs));
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
