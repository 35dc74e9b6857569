/* A plain-C99 client of the signal scan of include/soundscope_hip.h: four stereo streams of 2.5 tiles, stream 1 silent from its
 * frame 1000 on and with a run of five full-scale samples on its right channel, scanned without a pass; then the records and both
 * lists of stream 1.  Built and run by tests/test_signal_scan_abi.py (CPU: must fail loudly with SS_ERR_DEVICE).  Prints one line
 * of "key=value" pairs. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "soundscope_hip.h"

#define STREAMS 4u
#define FRAMES 10240u

int main(void)
{
    ss_batch_config cfg;
    ss_signal_scan_config scan;
    ss_batch *b = NULL;
    ss_stream_scan streams[STREAMS];
    ss_channel_scan channels[STREAMS * 2u];
    ss_signal_event silence[8], clips[8];
    uint32_t tile = 0u, cap = 0u, n_silence = 0u, n_clips = 0u;
    size_t i;
    int rc;
    float *pcm;
    memset(&cfg, 0, sizeof cfg);
    cfg.sample_rate = 48000; cfg.channels = 2; cfg.n_streams = STREAMS; cfg.fft_n = 4096; cfg.hop_frames = 1024;
    cfg.flags = SS_BATCH_TRUE_PEAK; cfg.frames_per_stream = FRAMES;
    memset(&scan, 0, sizeof scan);
    scan.silence_threshold = 0.0f; scan.clip_level = 1.0f; scan.silence_min_frames = 4800u; scan.clip_min_samples = 3u; scan.max_events = 8u;
    printf("abi=%d devices=%d sizeof_config=%u sizeof_stream=%u sizeof_channel=%u sizeof_event=%u ", ss_abi_version(), ss_device_count(),
           (unsigned)sizeof scan, (unsigned)sizeof streams[0], (unsigned)sizeof channels[0], (unsigned)sizeof silence[0]);
    rc = ss_batch_create(&cfg, &b);
    printf("create=%d", rc);
    if (rc == SS_OK) {
        pcm = (float *)malloc(sizeof(float) * STREAMS * FRAMES * 2u);
        if (!pcm) { printf(" run=%d\n", SS_ERR_NOMEM); ss_batch_destroy(b); return 0; }
        for (i = 0; i < (size_t)STREAMS * FRAMES * 2u; i++) pcm[i] = 0.25f;
        for (i = 1000u; i < FRAMES; i++) { pcm[(FRAMES + i) * 2u] = 0.0f; pcm[(FRAMES + i) * 2u + 1u] = 0.0f; }
        for (i = 500u; i < 505u; i++) pcm[(FRAMES + i) * 2u + 1u] = -1.0f;
        if ((rc = ss_batch_upload(b, 0u, STREAMS, pcm)) == SS_OK && (rc = ss_batch_signal_scan_plan(b, &tile, &cap)) == SS_OK &&
            (rc = ss_batch_signal_scan(b, &scan)) == SS_OK && (rc = ss_batch_download_stream_scans(b, streams, STREAMS)) == SS_OK &&
            (rc = ss_batch_download_channel_scans(b, channels, STREAMS * 2u)) == SS_OK &&
            (rc = ss_batch_download_signal_events(b, 1u, SS_SIGNAL_SILENCE, silence, 8u, &n_silence)) == SS_OK &&
            (rc = ss_batch_download_signal_events(b, 1u, SS_SIGNAL_CLIP, clips, 8u, &n_clips)) == SS_OK)
            printf(" tile=%u cap=%u trailing=%lu silence_runs=%lu n_silence=%u silence_at=%lu clip_runs=%lu n_clips=%u clip_at=%lu clip_frames=%lu"
                   " clip_channel=%u sum0=%.3f clean_runs=%lu",
                   (unsigned)tile, (unsigned)cap, (unsigned long)streams[1].trailing_silence, (unsigned long)streams[1].silence_runs,
                   (unsigned)n_silence, (unsigned long)(n_silence ? silence[0].first_frame : 0u), (unsigned long)streams[1].clip_runs,
                   (unsigned)n_clips, (unsigned long)(n_clips ? clips[0].first_frame : 0u), (unsigned long)(n_clips ? clips[0].frames : 0u),
                   (unsigned)(n_clips ? clips[0].channel : 0u), channels[0].sum, (unsigned long)(streams[0].silence_runs + streams[0].clip_runs));
        printf(" run=%d", rc);
        free(pcm);
        ss_batch_destroy(b);
    }
    printf("\n");
    return 0;
}
