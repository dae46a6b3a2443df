// raw2bcd.cpp -- the reference's raw-samples converter (src/raw_converter/main.cpp): `raw2bcd <input> <outputPrefix>` reads a raw file
// (20-byte header: int32 version, width, height, nbOfSamples, nbOfChannels in {3,4}; then the samples, pixel-major, all samples of a
// pixel contiguous, weight 1) and writes <prefix>.exr (mean colour, half), <prefix>_hist.exr (histograms + nbOfSamples as the last
// channel) and <prefix>_cov.exr (covariances): the inputs `bcd_cli -i <prefix>.exr` expects.  Histograms: 20 bins, gamma 2.2, max 2.5.
// The file streams through the device accumulator (bcd_hip_accum_add_dense) in row chunks, so host and device memory stay bounded and
// files larger than HBM convert; the disk read of chunk i+1 runs while the device copies and accumulates chunk i.
// Unlike the reference, which reads past a bad header silently, a truncated or inconsistent header, nbOfChannels outside {3,4},
// a non-positive size and a file shorter than its header claims are refused (rc 1) before the device is touched.
// Extra flags of this build: --chunk-mb <n> (size of a chunk, default 256); --save-state <file> writes the accumulator's state (format
// v1, bcd_hip.h) after everything else has been added; --merge-state <file> (repeatable) adds a state after the raw file, in command-line
// order -- with at least one of them <input> may be left out, the first state is then imported.  State files are checked (header, size,
// frame size, 20 bins, gamma 2.2, max 2.5) before the device is touched, and mapped rather than read.
#include "DeepImage.h"
#include "ImageIO.h"
#include "Utils.h"
#include "bcd_hip.h"

#include <hip/hip_runtime_api.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
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
		cout << "Usage: " << g_pProgramName << " [--chunk-mb <n>] [--save-state <file>] [--merge-state <file>]... <input> <outputPrefix>" << endl;
		cout << "       " << g_pProgramName << " [--save-state <file>] --merge-state <file> [--merge-state <file>]... <outputPrefix>" << endl;
		cout << "Converts a raw file with all samples into the inputs for the BayesianCollaborativeDenoiser program" << endl;
		cout << "Required arguments list:" << endl;
		cout << "    <input>           The file path to the input raw file" << endl;
		cout << "    <outputPrefix>    The file path to the output image, without .exr extension" << endl;
		cout << "Optional arguments list:" << endl;
		cout << "    --chunk-mb <n>    Megabytes of samples streamed to the device at a time (default: 256)" << endl;
		cout << "    --save-state <f>  Write the accumulator's state to <f> after everything has been added" << endl;
		cout << "    --merge-state <f> Add the accumulator state <f> after the raw file (repeatable, in order); without <input>" << endl;
		cout << "                      the first state is loaded and the others are added" << endl;
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

	// the raw file's header and size, checked before the device is touched; on success f is positioned at the first sample
	int openRaw(const string& i_rInput, FILE*& o_f, RawFileHeader& h, int64_t& o_rowBytes)
	{
		FILE* f = fopen(i_rInput.c_str(), "rb");
		if(!f)
			return error("cannot open input file '" + i_rInput + "'");
		o_f = f;
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
		o_rowBytes = rowBytes;
		return 0;
	}

	// a --merge-state file: header and exact size (format v1, bcd_hip.h), the frame size (io_W, io_H; taken from the file when < 0) and
	// raw2bcd's histogram parameters.  Host only.
	int checkState(const string& i_rPath, int& io_W, int& io_H)
	{
		FILE* f = fopen(i_rPath.c_str(), "rb");
		if(!f)
			return error("cannot open state file '" + i_rPath + "'");
		unsigned char raw[BCD_HIP_ACCUM_STATE_HEADER_BYTES];
		const size_t got = fread(raw, 1, sizeof(raw), f);
		const int64_t fileBytes = fseeko(f, 0, SEEK_END) == 0 ? int64_t(ftello(f)) : -1;
		fclose(f);
		if(got != sizeof(raw))
			return error("state file '" + i_rPath + "' is shorter than its 64-byte header");
		bcd_hip_accum_state_header hd;
		if(bcd_hip_accum_state_info(raw, fileBytes, &hd) != BCD_HIP_OK)
		{
			bcd_hip_accum_state_header claimed;
			std::memcpy(&claimed, raw, sizeof(claimed));
			const int64_t want = BCD_HIP_ACCUM_STATE_HEADER_BYTES + 4 * int64_t(claimed.nb_planes) * int64_t(claimed.width) * int64_t(claimed.height);
			if(claimed.width > 0 && claimed.height > 0 && bcd_hip_accum_state_info(raw, want, nullptr) == BCD_HIP_OK)
				return error("state file '" + i_rPath + "' is " + to_string(fileBytes) + " bytes, its header claims " + to_string(want));
			return error("'" + i_rPath + "' is not an accumulator state of format v1 (magic, version, sizes, bins, planes, reserved bytes or counters)");
		}
		if(io_W < 0)
		{
			io_W = hd.width;
			io_H = hd.height;
		}
		if(hd.width != io_W || hd.height != io_H)
			return error("state file '" + i_rPath + "' holds a " + to_string(hd.width) + " x " + to_string(hd.height) + " frame, the others " +
					to_string(io_W) + " x " + to_string(io_H));
		const float gamma = 2.2f, maxValue = 2.5f;
		if(hd.nb_bins != 20 || std::memcmp(&hd.gamma, &gamma, sizeof(float)) != 0 || std::memcmp(&hd.max_value, &maxValue, sizeof(float)) != 0)
			return error("state file '" + i_rPath + "' has " + to_string(hd.nb_bins) + " bins, gamma " + to_string(hd.gamma) + ", max " +
					to_string(hd.max_value) + "; raw2bcd accumulates 20 bins, gamma 2.2, max 2.5");
		return 0;
	}

	// read-only or writable mapping of a whole file
	struct Mapping
	{
		void* p = MAP_FAILED;
		size_t bytes = 0;
		~Mapping() { if(p != MAP_FAILED) munmap(p, bytes); }
	};

	bool mapForReading(const string& i_rPath, Mapping& o_m)
	{
		const int fd = open(i_rPath.c_str(), O_RDONLY);
		struct stat sb;
		if(fd < 0 || fstat(fd, &sb) != 0 || sb.st_size <= 0)
		{
			if(fd >= 0) close(fd);
			return false;
		}
		o_m.bytes = size_t(sb.st_size);
		o_m.p = mmap(nullptr, o_m.bytes, PROT_READ, MAP_PRIVATE, fd, 0);
		close(fd);
		if(o_m.p != MAP_FAILED)
			(void)madvise(o_m.p, o_m.bytes, MADV_SEQUENTIAL);
		return o_m.p != MAP_FAILED;
	}

	bool mapForWriting(const string& i_rPath, size_t i_bytes, Mapping& o_m)
	{
		const int fd = open(i_rPath.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
		if(fd < 0)
			return false;
		// blocks reserved first: a full disk fails here rather than on a page of the mapping
		if(posix_fallocate(fd, 0, off_t(i_bytes)) == 0)
		{
			o_m.bytes = i_bytes;
			o_m.p = mmap(nullptr, i_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
		}
		close(fd);
		return o_m.p != MAP_FAILED;
	}

	int convert(const string& i_rInput, const string& i_rPrefix, long long i_chunkMB, const vector<string>& i_rMergeStates, const string& i_rSaveState)
	{
		FILE* f = nullptr;
		struct Closer { FILE*& f; ~Closer() { if(f) fclose(f); } } closer{ f };
		RawFileHeader h = {};
		int64_t rowBytes = 0;
		int W = -1, H = -1;
		if(!i_rInput.empty())
		{
			if(int rc = openRaw(i_rInput, f, h, rowBytes))
				return rc;
			W = h.width;
			H = h.height;
		}
		for(const string& s : i_rMergeStates)
			if(int rc = checkState(s, W, H))
				return rc;

		if(f)
		{
			cout << "Version: " << h.version << endl;
			cout << "Resolution: " << h.width << "x" << h.height << endl;
			cout << "Nb of samples: " << h.nbOfSamples << endl;
			cout << "Nb of channels: " << h.nbOfChannels << endl;
		}
		else
			cout << "Resolution: " << W << "x" << H << " (from the state files)" << endl;

		const int nbOfBins = 20;
		const size_t npix = size_t(W) * H, D = 3 * nbOfBins;

		Resources r;
		if(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess)
			return error("no usable HIP device");
		if(bcd_hip_ctx_create(&r.ctx, 0, r.stream) != BCD_HIP_OK)
			return error("bcd_hip_ctx_create failed");
		if(bcd_hip_accum_create(r.ctx, W, H, nbOfBins, 2.2f, 2.5f, 0, &r.acc) != BCD_HIP_OK)
			return error(string("bcd_hip_accum_create: ") + bcd_hip_last_error(r.ctx));
		if(hipMalloc((void**)&r.stats, npix * (10 + D) * sizeof(float)) != hipSuccess)
			return error("out of device memory for the statistics");

		if(f)
		{
			const int rowsPerChunk = int(max<int64_t>(1, min<int64_t>(H, i_chunkMB * (int64_t(1) << 20) / rowBytes)));
			const size_t chunkBytes = size_t(rowsPerChunk) * size_t(rowBytes);
			for(int i = 0; i < 2; ++i)
				if(hipHostMalloc(&r.host[i], chunkBytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&r.dev[i], chunkBytes) != hipSuccess
						|| hipEventCreateWithFlags(&r.copied[i], hipEventDisableTiming) != hipSuccess)
					return error("out of memory for two chunks of " + to_string(chunkBytes) + " bytes");

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
			cout << "Converted in " << chunk << " chunk(s) of up to " << rowsPerChunk << " line(s)" << endl;
		}

		// the states after the raw file, in command-line order; without a raw file the first one is imported
		for(size_t i = 0; i < i_rMergeStates.size(); ++i)
		{
			const string& s = i_rMergeStates[i];
			Mapping m;
			if(!mapForReading(s, m))
				return error("cannot map state file '" + s + "'");
			const bool import = !f && i == 0;
			const int rc = import ? bcd_hip_accum_import(r.acc, m.p, int64_t(m.bytes)) : bcd_hip_accum_merge_state(r.acc, m.p, int64_t(m.bytes));
			if(rc != BCD_HIP_OK)
				return error(string(import ? "bcd_hip_accum_import" : "bcd_hip_accum_merge_state") + " of '" + s + "': " + bcd_hip_last_error(r.ctx));
			cout << (import ? "Imported state " : "Merged state ") << s << endl;
		}

		if(!i_rSaveState.empty())
		{
			int64_t bytes = 0;
			Mapping m;
			if(bcd_hip_accum_state_bytes(r.acc, &bytes) != BCD_HIP_OK || !mapForWriting(i_rSaveState, size_t(bytes), m))
				return error("cannot write the state to '" + i_rSaveState + "': " + strerror(errno));
			if(bcd_hip_accum_export(r.acc, m.p, bytes) != BCD_HIP_OK)
				return error(string("bcd_hip_accum_export to '") + i_rSaveState + "': " + bcd_hip_last_error(r.ctx));
			cout << "Saved state " << i_rSaveState << " (" << bytes << " bytes)" << endl;
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
	vector<string> positional, mergeStates;
	string saveState;
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
		else if(a == "--save-state" || a == "--merge-state")
		{
			if(i + 1 >= argc || argv[i + 1][0] == '\0')
			{
				printUsage();
				return error(a + " takes a file path");
			}
			if(a == "--save-state")
				saveState = argv[++i];
			else
				mergeStates.push_back(argv[++i]);
		}
		else
			positional.push_back(a);
	}
	// <input> may be left out when at least one state is merged
	if(positional.size() == 1 && !mergeStates.empty())
		positional.insert(positional.begin(), string());
	if(positional.size() != 2)
	{
		printUsage();
		return 1;
	}
	return convert(positional[0], positional[1], chunkMB, mergeStates, saveState);
}
