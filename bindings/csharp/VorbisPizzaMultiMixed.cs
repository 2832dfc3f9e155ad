// P/Invoke binding of include/vorbispizza_multi_mixed.h -- the dispatcher of VorbisPizzaMulti.cs with streams of different
// setup headers in one device-decoded sub-batch, and the counts of the last call.  A host creates its dispatcher as before
// (VorbisPizzaMulti.vpzm_create with GpuEntropy != 0), turns the option on once and decodes its libraries; the PCM and the
// results are the same bit for bit, a library of many setups takes fewer, larger calls.  Style of
// NVorbis.Tests/Bindings/Vorbisfile.cs:43-107.
using System;
using System.Runtime.InteropServices;

namespace NVorbis.Native
{
    public static unsafe class VorbisPizzaMultiMixed
    {
        private const string Host = "vorbispizza_host";

        [StructLayout(LayoutKind.Sequential)]
        public struct CallCounts                      // vpzm_call_counts: of the last vpzm_decode_library call, all groups
        {
            public long SubBatches;
            public long DeviceDecodedSubBatches;      // ... those that were entropy-decoded on the device
            public long MixedSubBatches;              // sub-batches whose members have two or more different setups
            public long MaxSetupsPerSubBatch;
            public long DecodersCreated;              // vpz_decoder_create calls of that call
            public fixed long Reserved[3];
        }

        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_set_mixed_setups(VorbisPizzaMulti.DispatcherHandle m, int on);
        [DllImport(Host, CallingConvention = CallingConvention.Cdecl)] public static extern int vpzm_last_call_counts(VorbisPizzaMulti.DispatcherHandle m, out CallCounts counts);
    }
}
