// P/Invoke binding of include/vorbispizza_pcm_normalize.h -- windows of a planar float32 device array (channel c of a window lies
// c * frames elements behind its channel 0: the tensor [rows][channels][frames] of GpuPcmResample's planar layout) delivered as a dense,
// zero-padded batch whose rows are normalised on the way: zero mean and unit variance over a row's REAL samples (wav2vec 2.0's
// feature extractor), a peak level, an RMS level or a gain per row, with an optional ceiling on the delivered peak; float32 or int16,
// planar or frames-major.  A host fills one NormRow per row and a NormSpec, asks vpz_pcm_normalize_scratch for the float64 elements of
// scratch memory and makes one vpz_pcm_normalize call, asynchronous on the context's stream; an optional device array of NormResult
// takes every row's sums, peak, offset and gain.  The header states the definition, the order of the sums and the error bound.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmNormalize
    {
        private const string Synth = "vorbispizza_synth";

        public const int NormMeanvar = 1, NormPeak = 2, NormRms = 3, NormGain = 4;  // NormSpec.Mode
        public const int NormChunk = 1024;                                          // VPZ_NORM_CHUNK

        [StructLayout(LayoutKind.Sequential)]
        public struct NormRow
        {
            public long Src;
            public long Samples;
            public long Row;
            public double Gain;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct NormSpec
        {
            public double Target;
            public double Eps;
            public double Ceiling;
            public int Mode;
            public int Channels;
            public fixed int Reserved[8];
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct NormResult
        {
            public double Sum;
            public double SumSq;
            public double Peak;
            public double Mean;
            public double Gain;
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_normalize_scratch(int nRows, int channels, long frames, long* doubles);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_normalize(IntPtr ctx, void* srcDev, long srcElems, long frames, NormSpec* spec, int nRows, NormRow* rows, void* dstDev, long dstRows, int dstLayout, void* scratchDev, long scratchDoubles, NormResult* resultDev);
    }
}
