// P/Invoke binding of include/vorbispizza_pcm_logmel.h -- windows of a MONO float32 device PCM array delivered as (log-)mel feature
// frames in device memory: framing with reflection at both ends, periodic Hann window, DFT, power, mel filterbank, log10, in one launch
// and with no spectrogram in device memory.  A host that has the mono rows of GpuPcmResample.vpz_pcm_resample (downmix 1, planar
// float32) fills one GpuPcmPack.PackRow per window -- where it starts, how many samples it has, which row it becomes -- and a LogMelSpec,
// and makes one vpz_pcm_logmel call: every named row gets 1 + frames / hop feature frames of nMels bands, asynchronously on the
// context's stream.  The header states the definition (torch.stft with center and reflect, torchaudio's melscale_fbanks);
// vpz_logmel_dft_table and vpz_mel_filterbank give the tables without a device.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmLogMel
    {
        private const string Synth = "vorbispizza_synth";

        public const int LogMelMinNfft = 32;          // VPZ_LOGMEL_MIN_NFFT: n_fft even, 32 ..
        public const int LogMelMaxNfft = 1024;        // VPZ_LOGMEL_MAX_NFFT: .. 1024
        public const int LogMelMaxMels = 256;         // VPZ_LOGMEL_MAX_MELS
        public const int MelHtk = 0, MelSlaney = 1;               // LogMelSpec.MelScale
        public const int MelNormNone = 0, MelNormSlaney = 1;      // LogMelSpec.MelNorm
        public const int MelPower = 0, MelLog10 = 1;              // LogMelSpec.Output
        public const int MelBandsFirst = 0, MelFramesFirst = 1;   // LogMelSpec.Layout: [rows][nMels][T] or [rows][T][nMels]

        [StructLayout(LayoutKind.Sequential)]
        public struct LogMelSpec
        {
            public double SampleRate;
            public double FMin, FMax;
            public double Floor;
            public int NFft;
            public int Hop;
            public int NMels;
            public int MelScale;
            public int MelNorm;
            public int Output;
            public int Layout;
            public fixed int Reserved[9];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_logmel_dft_table(int nFft, float* table, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_mel_filterbank(LogMelSpec* spec, int* firstBin, int* nBins, float* weights, long capacity, long* total);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_logmel(IntPtr ctx, void* srcDev, long srcElems, long frames, LogMelSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
