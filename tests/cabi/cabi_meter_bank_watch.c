/* A plain-C99 client of the meter banks' signal watch of include/soundscope_hip.h: a bank of two stereo meters with the watch on,
 * two blocks of 10 ms — stream 0 falls silent at frame 100 of the first, stream 1 clips five samples of its right channel in each —
 * the records after both, a selective reset, the watch off.  Built and run by tests/test_meter_bank_watch_abi.py (CPU: must fail
 * loudly with SS_ERR_DEVICE).  Prints one line of "key=value" pairs. */
#include <stdio.h>

#include "soundscope_hip.h"

int main(void)
{
    enum { N = 2, C = 2, FRAMES = 480 };
    static float pcm[N * FRAMES * C];
    const ss_signal_scan_config cfg = {0.0f, 1.0f, 48u, 3u, 0u, 0u};
    ss_signal_scan_config listed = {0.0f, 1.0f, 48u, 3u, 8u, 0u};
    ss_stream_watch st[N];
    ss_channel_watch ch[N * C];
    const uint32_t one = 1u;
    ss_meter_bank *m = NULL;
    uint32_t tile = 0;
    unsigned i;
    int rc;
    for (i = 0; i < N * FRAMES * C; i++) pcm[i] = 0.25f;
    for (i = 100 * C; i < FRAMES * C; i++) pcm[i] = 0.0f;
    for (i = 50; i < 55; i++) pcm[(FRAMES + i) * C + 1] = -1.0f;
    printf("abi=%d devices=%d sizeof_stream=%u sizeof_channel=%u ", ss_abi_version(), ss_device_count(), (unsigned)sizeof(ss_stream_watch),
           (unsigned)sizeof(ss_channel_watch));
    rc = ss_meter_bank_create(N, C, 48000u, 0, &m);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        printf(" before=%d", ss_meter_bank_signal_watch(m, st, N, ch, N * C));
        printf(" events=%d", ss_meter_bank_signal_watch_enable(m, &listed));
        if ((rc = ss_meter_bank_signal_watch_enable(m, &cfg)) == SS_OK && (rc = ss_meter_bank_signal_watch_plan(m, &tile)) == SS_OK &&
            (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK && (rc = ss_meter_bank_add(m, pcm, FRAMES)) == SS_OK &&
            (rc = ss_meter_bank_signal_watch(m, st, N, ch, N * C)) == SS_OK)
            printf(" tile=%u frames=%lu trailing=%lu silence_runs=%lu longest_at=%lu clip_runs=%lu last_clip=%lu sum0=%g small=%d", tile,
                   (unsigned long)st[0].frames, (unsigned long)st[0].trailing_silence, (unsigned long)st[0].silence_runs,
                   (unsigned long)st[0].longest_silence_at, (unsigned long)st[1].clip_runs, (unsigned long)ch[3].last_clip_frame, ch[0].sum,
                   ss_meter_bank_signal_watch(m, st, N - 1, NULL, 0));
        if (rc == SS_OK && (rc = ss_meter_bank_signal_watch_reset(m, &one, 1)) == SS_OK &&
            (rc = ss_meter_bank_signal_watch(m, st, N, NULL, 0)) == SS_OK)
            printf(" kept=%lu after_reset=%lu", (unsigned long)st[0].frames, (unsigned long)st[1].frames);
        printf(" run=%d off=%d", rc, ss_meter_bank_signal_watch_enable(m, NULL));
        printf(" after=%d", ss_meter_bank_signal_watch_plan(m, &tile));
        ss_meter_bank_destroy(m);
    }
    printf("\n");
    return 0;
}
