// P/Invoke binding of include/vorbispizza_pcm_loudness.h -- windows of an interleaved float32 device PCM array measured for programme
// loudness (ITU-R BS.1770-4 / EBU R 128) on the device: the K-weighting filter in float64, the sum of squares of every 100 ms step and
// the sample peak of every window, in device memory; the gate of the integrated value runs on the host.  A host that has the PCM of a
// synth call with VPZ_OUT_INTERLEAVED in device memory fills one GpuPcmPack.PackRow per window -- where it starts, how many samples it
// has, which row it becomes --, takes the weights of vpz_loudness_weights and makes one vpz_pcm_loudness call per sample rate: row r of
// sumsDev[dstRows][maxSteps] (double) gets the window's step sums and +0.0 behind them, peakDev[r] (float) its peak, asynchronously on
// the context's stream.  vpz_loudness_gate turns a row's first samples / S sums (S = (rate + 5) / 10) into the integrated LUFS.  The
// header states the definition; vpz_loudness_filter gives the coefficients of a rate without a device.
// Out of scope: true peak, loudness range, short-term values, int16 sources, a gain on delivery.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmLoudness
    {
        private const string Synth = "vorbispizza_synth";

        public const int LoudnessMinRate = 8000;     // VPZ_LOUDNESS_MIN_RATE
        public const int LoudnessMaxRate = 384000;   // VPZ_LOUDNESS_MAX_RATE

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_loudness_filter(int sampleRate, double* coeffs);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_loudness_weights(int channels, double* w);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_loudness(IntPtr ctx, void* srcDev, long srcElems, int channels, int sampleRate, double* weights, int nRows, GpuPcmPack.PackRow* rows, double* sumsDev, float* peakDev, long dstRows, long maxSteps);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_loudness_gate(double* sums, long nSteps, int stepLen, double* lufs, long* blocksKept);
    }
}
