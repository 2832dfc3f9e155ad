// P/Invoke binding of include/vorbispizza_pcm_mfcc.h -- windows of a MONO float32 device PCM array delivered as Kaldi MFCC feature
// frames in device memory: the log-mel values of GpuPcmFbank.cs (bit for bit), the liftered DCT over them, C0 replaced by the frame's raw
// log energy, HTK's coefficient order, and cepstral mean subtraction over a row's real frames.  A host that has the mono rows of
// GpuPcmResample.vpz_pcm_resample (downmix 1, planar float32) fills one GpuPcmPack.PackRow per window and an MfccSpec -- its Fbank member
// is the mel stage's spec, Output = FbankLog; Layout and PadValue are the cepstral tensor's -- and makes one vpz_pcm_mfcc call: every
// named row gets 1 + (frames - win) / hop feature frames of NCeps coefficients, asynchronously on the context's stream; the frames behind
// a row's real ones hold PadValue.  The header states the definition (torchaudio.compliance.kaldi.mfcc without dither and VTLN, raw
// energy); vpz_mfcc_table gives the cepstral matrix, in the stored order, without a device.
// Style of NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class GpuPcmMfcc
    {
        private const string Synth = "vorbispizza_synth";

        [StructLayout(LayoutKind.Sequential)]
        public struct MfccSpec
        {
            public GpuPcmFbank.FbankSpec Fbank;
            public double Lifter;
            public double EnergyFloor;
            public int NCeps;
            public int UseEnergy;
            public int HtkCompat;
            public int SubtractMean;
            public fixed int Reserved[12];
        }

        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_mfcc_table(MfccSpec* spec, float* table, long capacity);
        [DllImport(Synth, CallingConvention = CallingConvention.Cdecl)] public static extern int vpz_pcm_mfcc(IntPtr ctx, void* srcDev, long srcElems, long frames, MfccSpec* spec, int nRows, GpuPcmPack.PackRow* rows, void* dstDev, long dstRows);
    }
}
