// P/Invoke binding of include/vorbispizza_pcm_melspec.h -- windows of a MONO float32 device PCM array delivered as (log-)mel spectrogram
// frames with transforms of 2048, 4096 and 8192 samples: framing with reflection at both ends, periodic Hann window, one real FFT per
// frame in LDS, power, mel filterbank, log10, in one launch and with no spectrogram in device memory.  The spec is
// GpuPcmLogMel.LogMelSpec and the descriptors are GpuPcmPack.PackRow: the call is vpz_pcm_logmel's for the mel front ends of music
// models.  The header states the definition, the network and its error bound; vpz_melspec_twiddles and vpz_melspec_filterbank give the
// tables without a device.  Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmMelspec
    {
        private const string Synth = "vorbispizza_synth";

        public const int MelspecMinNfft = 2048;       // VPZ_MELSPEC_MIN_NFFT: n_fft 2048, 4096 ..
        public const int MelspecMaxNfft = 8192;       // VPZ_MELSPEC_MAX_NFFT: .. or 8192
        public const int MelspecMaxMels = 256;        // VPZ_MELSPEC_MAX_MELS

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_melspec_twiddles(int nFft, float* table, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_melspec_filterbank(GpuPcmLogMel.LogMelSpec* spec, int* firstBin, int* nBins, float* weights, long capacity, long* total);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_melspec(IntPtr ctx, void* srcDev, long srcElems, long frames, GpuPcmLogMel.LogMelSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
