// raw2bcd.cpp -- the reference's raw-samples converter (src/raw_converter/main.cpp): `raw2bcd <input> <outputPrefix>` reads a raw file
// (20-byte header: int32 version, width, height, nbOfSamples, nbOfChannels in {3,4}; then the samples, pixel-major, all samples of a
// pixel contiguous, weight 1) and writes <prefix>.exr (mean colour, half), <prefix>_hist.exr (histograms + nbOfSamples as the last
// channel) and <prefix>_cov.exr (covariances): the inputs `bcd_cli -i <prefix>.exr` expects.  Histograms: 20 bins, gamma 2.2, max 2.5.
// The file streams through the device accumulator (bcd_hip_accum_add_dense) in row chunks, so host and device memory stay bounded and
// files larger than HBM convert; the disk read of chunk i+1 runs while the device copies and accumulates chunk i.
// Unlike the reference, which reads past a bad header silently, a truncated or inconsistent header, nbOfChannels outside {3,4},
// a non-positive size and a file shorter than its header claims are refused (rc 1) before the device is touched.
// Extra flag of this build: --chunk-mb <n> (size of a chunk, default 256).
#include "DeepImage.h"
#include "ImageIO.h"
#include "Utils.h"
#include "bcd_hip.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace std;
using namespace bcd;

namespace
{

	const char* g_pProgramName = "raw2bcd";

	struct RawFileHeader
	{
		int32_t version, width, height, nbOfSamples, nbOfChannels;
	};

	void printUsage()
	{
		cout << "raw2bcd (MI355X / HIP build)" << endl << endl;
		cout << "Usage: " << g_pProgramName << " [--chunk-mb <n>] <input> <outputPrefix>" << endl;
		cout << "Converts a raw file with all samples into the inputs for the BayesianCollaborativeDenoiser program" << endl;
		cout << "Required arguments list:" << endl;
		cout << "    <input>           The file path to the input raw file" << endl;
		cout << "    <outputPrefix>    The file path to the output image, without .exr extension" << endl;
		cout << "Optional arguments list:" << endl;
		cout << "    --chunk-mb <n>    Megabytes of samples streamed to the device at a time (default: 256)" << endl;
	}

	int error(const string& i_rMessage)
	{
		cerr << "Error in program '" << g_pProgramName << "': " << i_rMessage << endl;
		return 1;
	}

	struct Resources
	{
		hipStream_t stream = nullptr;
		bcd_hip_ctx* ctx = nullptr;
		bcd_hip_accum* acc = nullptr;
		void* host[2] = { nullptr, nullptr };
		void* dev[2] = { nullptr, nullptr };
		hipEvent_t copied[2] = { nullptr, nullptr };
		float* stats = nullptr;
		~Resources()
		{
			if(stream) (void)hipStreamSynchronize(stream);
			bcd_hip_accum_destroy(acc);
			bcd_hip_ctx_destroy(ctx);
			for(int i = 0; i < 2; ++i)
			{
				if(host[i]) (void)hipHostFree(host[i]);
				if(dev[i]) (void)hipFree(dev[i]);
				if(copied[i]) (void)hipEventDestroy(copied[i]);
			}
			if(stats) (void)hipFree(stats);
			if(stream) (void)hipStreamDestroy(stream);
		}
	};

	int convert(const string& i_rInput, const string& i_rPrefix, long long i_chunkMB)
	{
		FILE* f = fopen(i_rInput.c_str(), "rb");
		if(!f)
			return error("cannot open input file '" + i_rInput + "'");
		struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{ f };
		RawFileHeader h;
		if(fread(&h, 1, sizeof(h), f) != sizeof(h))
			return error("truncated header: a raw file starts with 20 bytes (int32 version, width, height, nbOfSamples, nbOfChannels)");
		if(h.nbOfChannels != 3 && h.nbOfChannels != 4)
			return error("nbOfChannels is " + to_string(h.nbOfChannels) + ", must be 3 or 4");
		if(h.width <= 0 || h.height <= 0 || h.nbOfSamples <= 0)
			return error("width, height and nbOfSamples must be positive (header: " + to_string(h.width) + " x " + to_string(h.height) + ", " +
					to_string(h.nbOfSamples) + " samples)");
		if(int64_t(h.width) * h.height >= (int64_t(1) << 31))
			return error("more than 2^31 pixels");
		const int64_t rowBytes = int64_t(h.width) * h.nbOfSamples * h.nbOfChannels * int64_t(sizeof(float)); // < 2^64: each factor < 2^31
		if(rowBytes > (int64_t(1) << 40) / h.height)
			return error("header claims more than 1 TiB of samples");
		const int64_t payload = rowBytes * h.height;
		if(fseeko(f, 0, SEEK_END) != 0)
			return error("cannot seek in '" + i_rInput + "'");
		const int64_t fileBytes = ftello(f);
		if(fileBytes < int64_t(sizeof(h)) + payload)
			return error("file is " + to_string(fileBytes) + " bytes, its header claims " + to_string(int64_t(sizeof(h)) + payload));
		if(fseeko(f, sizeof(h), SEEK_SET) != 0)
			return error("cannot seek in '" + i_rInput + "'");
		if(fileBytes > int64_t(sizeof(h)) + payload)
			cerr << "Warning: " << fileBytes - int64_t(sizeof(h)) - payload << " bytes after the samples are ignored" << endl;

		cout << "Version: " << h.version << endl;
		cout << "Resolution: " << h.width << "x" << h.height << endl;
		cout << "Nb of samples: " << h.nbOfSamples << endl;
		cout << "Nb of channels: " << h.nbOfChannels << endl;

		const int W = h.width, H = h.height, nbOfBins = 20;
		const int rowsPerChunk = int(max<int64_t>(1, min<int64_t>(H, i_chunkMB * (int64_t(1) << 20) / rowBytes)));
		const size_t chunkBytes = size_t(rowsPerChunk) * size_t(rowBytes);
		const size_t npix = size_t(W) * H, D = 3 * nbOfBins;

		Resources r;
		if(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess)
			return error("no usable HIP device");
		if(bcd_hip_ctx_create(&r.ctx, 0, r.stream) != BCD_HIP_OK)
			return error("bcd_hip_ctx_create failed");
		if(bcd_hip_accum_create(r.ctx, W, H, nbOfBins, 2.2f, 2.5f, 0, &r.acc) != BCD_HIP_OK)
			return error(string("bcd_hip_accum_create: ") + bcd_hip_last_error(r.ctx));
		for(int i = 0; i < 2; ++i)
			if(hipHostMalloc(&r.host[i], chunkBytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&r.dev[i], chunkBytes) != hipSuccess
					|| hipEventCreateWithFlags(&r.copied[i], hipEventDisableTiming) != hipSuccess)
				return error("out of memory for two chunks of " + to_string(chunkBytes) + " bytes");
		if(hipMalloc((void**)&r.stats, npix * (10 + D) * sizeof(float)) != hipSuccess)
			return error("out of device memory for the statistics");

		bool inFlight[2] = { false, false };
		int chunk = 0;
		for(int line = 0; line < H; line += rowsPerChunk, ++chunk)
		{
			const int b = chunk & 1, rows = min(rowsPerChunk, H - line);
			const size_t bytes = size_t(rows) * size_t(rowBytes);
			if(inFlight[b] && hipEventSynchronize(r.copied[b]) != hipSuccess) // (the copy of chunk - 2 has left this pinned buffer)
				return error("device copy failed");
			if(fread(r.host[b], 1, bytes, f) != bytes)
				return error("read error in '" + i_rInput + "'");
			// the device buffer of chunk - 2 is free: its accumulation is ahead of this copy on the stream
			if(hipMemcpyAsync(r.dev[b], r.host[b], bytes, hipMemcpyHostToDevice, r.stream) != hipSuccess || hipEventRecord(r.copied[b], r.stream) != hipSuccess)
				return error("device copy failed");
			inFlight[b] = true;
			if(bcd_hip_accum_add_dense(r.acc, (const float*)r.dev[b], nullptr, line, rows, h.nbOfSamples, h.nbOfChannels) != BCD_HIP_OK)
				return error(string("bcd_hip_accum_add_dense: ") + bcd_hip_last_error(r.ctx));
		}

		Deepimf ns(W, H, 1), mean(W, H, 3), cov(W, H, 6), hist(W, H, int(D));
		float* d = r.stats;
		if(bcd_hip_accum_statistics(r.acc, d, d + npix, d + 4 * npix, d + 10 * npix) != BCD_HIP_OK)
			return error(string("bcd_hip_accum_statistics: ") + bcd_hip_last_error(r.ctx));
		if(hipMemcpyAsync(ns.getDataPtr(), d, npix * sizeof(float), hipMemcpyDeviceToHost, r.stream) != hipSuccess
				|| hipMemcpyAsync(mean.getDataPtr(), d + npix, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, r.stream) != hipSuccess
				|| hipMemcpyAsync(cov.getDataPtr(), d + 4 * npix, npix * 6 * sizeof(float), hipMemcpyDeviceToHost, r.stream) != hipSuccess
				|| hipMemcpyAsync(hist.getDataPtr(), d + 10 * npix, npix * D * sizeof(float), hipMemcpyDeviceToHost, r.stream) != hipSuccess
				|| hipStreamSynchronize(r.stream) != hipSuccess)
			return error("statistics download failed");
		cout << "Converted in " << chunk << " chunk(s) of up to " << rowsPerChunk << " line(s)" << endl;

		Deepimf histAndNs = Utils::mergeHistogramAndNbOfSamples(hist, ns);
		hist.clearAndFreeMemory();
		ns.clearAndFreeMemory();
		const string colorPath = i_rPrefix + ".exr", histPath = i_rPrefix + "_hist.exr", covPath = i_rPrefix + "_cov.exr";
		if(!ImageIO::writeEXR(mean, colorPath.c_str()))
			return error("cannot write '" + colorPath + "': " + ImageIO::lastError());
		if(!ImageIO::writeMultiChannelsEXR(cov, covPath.c_str()))
			return error("cannot write '" + covPath + "': " + ImageIO::lastError());
		if(!ImageIO::writeMultiChannelsEXR(histAndNs, histPath.c_str()))
			return error("cannot write '" + histPath + "': " + ImageIO::lastError());
		return 0;
	}

} // namespace

int main(int argc, const char** argv)
{
	vector<string> positional;
	long long chunkMB = 256;
	for(int i = 1; i < argc; ++i)
	{
		const string a = argv[i];
		if(a == "--chunk-mb")
		{
			char* end = nullptr;
			chunkMB = i + 1 < argc ? strtoll(argv[i + 1], &end, 10) : 0;
			if(i + 1 >= argc || *end != '\0' || chunkMB <= 0)
			{
				printUsage();
				return error("--chunk-mb takes a positive integer");
			}
			++i;
		}
		else
			positional.push_back(a);
	}
	if(positional.size() != 2)
	{
		printUsage();
		return 1;
	}
	return convert(positional[0], positional[1], chunkMB);
}
