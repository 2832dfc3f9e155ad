// P/Invoke binding of include/vorbispizza_pcm_stft.h -- windows of a float32 device PCM array delivered as short-time Fourier
// spectrograms in device memory, one row per descriptor: framing with reflection at both ends, a periodic Hann or Hamming window of
// winLength samples centred in nFft, one real FFT per frame in LDS (nFft 512 to 8192), and the spectrum itself stored -- complex pairs,
// magnitudes or power, bins first (torch.stft's order) or frames first.  The stage has no notion of channels: a host that has the planar
// rows of GpuPcmResample.vpz_pcm_resample (downmix 0, planar float32) fills one GpuPcmPack.PackRow per (window, channel) and a StftSpec,
// and makes one vpz_pcm_stft call, asynchronously on the context's stream.  The header states the definition, the network and its error
// bound; vpz_stft_table gives the window and the twiddles without a device.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmStft
    {
        private const string Synth = "vorbispizza_synth";

        public const int StftMinNfft = 512;           // VPZ_STFT_MIN_NFFT: n_fft 512, 1024, 2048, 4096 ..
        public const int StftMaxNfft = 8192;          // VPZ_STFT_MAX_NFFT: .. or 8192
        public const int StftHann = 0, StftHamming = 1;                     // StftSpec.Window
        public const int StftComplex = 0, StftMagnitude = 1, StftPower = 2; // StftSpec.Output
        public const int StftBinsFirst = 0, StftFramesFirst = 1;            // StftSpec.Layout: [rows][nFreq][T] or [rows][T][nFreq], (re, im) pairs for StftComplex

        [StructLayout(LayoutKind.Sequential)]
        public struct StftSpec
        {
            public int NFft;
            public int Hop;
            public int WinLength;
            public int Window;
            public int Output;
            public int Layout;
            public fixed int Reserved[10];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_stft_table(int nFft, int winLength, int window, float* table, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_stft(IntPtr ctx, void* srcDev, long srcElems, long frames, StftSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
