// P/Invoke binding of include/vorbispizza_pcm_fbank.h -- windows of a MONO float32 device PCM array delivered as Kaldi filterbank
// feature frames in device memory: snip_edges framing, per-frame mean removal and pre-emphasis, a Povey / Hamming / Hanning window
// shorter than the transform, power, Kaldi's mel bank, natural log, in one launch and with neither the framed batch nor a spectrogram in
// device memory.  A host that has the mono rows of GpuPcmResample.vpz_pcm_resample (downmix 1, planar float32) fills one
// GpuPcmPack.PackRow per window -- where it starts, how many samples it has, which row it becomes -- and an FbankSpec, and makes one
// vpz_pcm_fbank call: every named row gets 1 + (frames - win) / hop feature frames of nMels bands, asynchronously on the context's
// stream; the frames behind a row's real ones hold PadValue.  The header states the definition (torchaudio.compliance.kaldi.fbank
// without dither, VTLN and energy); vpz_fbank_table and vpz_fbank_filterbank give the tables without a device.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmFbank
    {
        private const string Synth = "vorbispizza_synth";

        public const int FbankMinNfft = 32;           // VPZ_FBANK_MIN_NFFT: n_fft even, 32 ..
        public const int FbankMaxNfft = 1024;         // VPZ_FBANK_MAX_NFFT: .. 1024
        public const int FbankMaxMels = 256;          // VPZ_FBANK_MAX_MELS
        public const int FbankHanning = 0, FbankHamming = 1, FbankPovey = 2;   // FbankSpec.Window
        public const int FbankPower = 0, FbankLog = 1;                         // FbankSpec.Output
        public const int FbankBandsFirst = 0, FbankFramesFirst = 1;            // FbankSpec.Layout: [rows][nMels][T] or [rows][T][nMels]

        [StructLayout(LayoutKind.Sequential)]
        public struct FbankSpec
        {
            public double SampleRate;
            public double LowFreq;
            public double HighFreq;
            public double Preemphasis;
            public double Scale;
            public double Floor;
            public double PadValue;
            public int Win;
            public int Hop;
            public int NFft;
            public int NMels;
            public int Window;
            public int RemoveDc;
            public int Output;
            public int Layout;
            public fixed int Reserved[10];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_fbank_table(FbankSpec* spec, float* table, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_fbank_filterbank(FbankSpec* spec, int* firstBin, int* nBins, float* weights, long capacity, long* total);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_fbank(IntPtr ctx, void* srcDev, long srcElems, long frames, FbankSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
