// P/Invoke binding of include/vorbispizza_pcm_cqt.h -- windows of a float32 device PCM array delivered as constant-Q (or variable-Q)
// spectrograms in device memory, one row per descriptor: geometrically spaced bins at fMin * 2^(k / binsPerOctave), one periodic Hann or
// Hamming window per bin, frames centred on sample t * hop with reflection or zeros beyond the row, and the transform itself stored --
// complex pairs, magnitudes or power, bins first or frames first.  The stage has no notion of channels: a host that has the planar rows of
// GpuPcmResample.vpz_pcm_resample (downmix 0, planar float32) fills one GpuPcmPack.PackRow per (window, channel) and a CqtSpec, and makes
// one vpz_pcm_cqt call, asynchronously on the context's stream.  The header states the definition and its error bound; vpz_cqt_bins and
// vpz_cqt_kernel give the bins and a bin's coefficients without a device.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmCqt
    {
        private const string Synth = "vorbispizza_synth";

        public const int CqtMaxBins = 512;            // VPZ_CQT_MAX_BINS
        public const int CqtMaxBinsPerOctave = 96;    // VPZ_CQT_MAX_BINS_PER_OCTAVE
        public const int CqtMaxLength = 65536;        // VPZ_CQT_MAX_LENGTH: the longest kernel, N_0
        public const int CqtMaxHop = 2048;            // VPZ_CQT_MAX_HOP
        public const int CqtHann = 0, CqtHamming = 1;                    // CqtSpec.Window
        public const int CqtScaleNone = 0, CqtScaleSqrtLength = 1;       // CqtSpec.Scale
        public const int CqtPadReflect = 0, CqtPadZero = 1;              // CqtSpec.Pad
        public const int CqtComplex = 0, CqtMagnitude = 1, CqtPower = 2; // CqtSpec.Output
        public const int CqtBinsFirst = 0, CqtFramesFirst = 1;           // CqtSpec.Layout: [rows][nBins][T] or [rows][T][nBins], (re, im) pairs for CqtComplex

        [StructLayout(LayoutKind.Sequential)]
        public struct CqtSpec
        {
            public double SampleRate;
            public double FMin;
            public double FilterScale;
            public double Gamma;
            public int NBins;
            public int BinsPerOctave;
            public int Hop;
            public int Window;
            public int Scale;
            public int Pad;
            public int Output;
            public int Layout;
            public fixed int Reserved[8];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_cqt_bins(CqtSpec* spec, double* freqs, int* lengths, int capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_cqt_kernel(CqtSpec* spec, int k, float* table, long capacity, int* length);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_cqt(IntPtr ctx, void* srcDev, long srcElems, long frames, CqtSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
