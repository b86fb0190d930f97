/*
 * permessage-deflate with the MI355X inflate: PerMessageDeflateExtension
 * (PerMessageDeflateExtension.java:45-328) negotiates exactly as the reference
 * (this class delegates offer / acceptOffer / validateResponse / response to it),
 * and the negotiated extension's updateDecoders puts the reference
 * PerMessageDeflateDecoder after "ws-decoder" (:316-326), which is then wrapped
 * in a GpuPerMessageDeflateDecoder under the same key.  The decoder's noContext is
 * the negotiated one: the client's no_context_takeover for a server, the server's
 * for a client (:321-325), read back from the response parameters.  Compression:
 * updateEncoders puts the reference PerMessageDeflateEncoder after "ws-encoder"
 * (:303-313), which is then wrapped in a GpuPerMessageDeflateEncoder under the same key
 * ("permessage-deflate-encoder") with the negotiated noContext (the server's
 * server_no_context_takeover for a server, the client's for a client, :310) and the
 * compression level; behind a GpuFrameEncoder it compresses in that encoder's device
 * batch.  The level: the one given here (PerMessageDeflateExtension keeps its own
 * private), 6 by default as PerMessageDeflateExtension() (:144-146).
 *
 * GpuHandshakeNegotiator (below) carries the same extension's settings to the
 * handshake natives that negotiate on the device.
 */
package org.snf4j.websocket.gpu;

import java.nio.ByteBuffer;
import java.nio.charset.StandardCharsets;
import java.util.List;

import org.snf4j.core.codec.ICodec;
import org.snf4j.core.codec.ICodecPipeline;
import org.snf4j.websocket.extensions.IExtension;
import org.snf4j.websocket.extensions.InvalidExtensionException;
import org.snf4j.websocket.IWebSocketSessionConfig;
import org.snf4j.websocket.extensions.compress.PerMessageDeflateDecoder;
import org.snf4j.websocket.extensions.compress.PerMessageDeflateEncoder;
import org.snf4j.websocket.extensions.compress.PerMessageDeflateExtension;
import org.snf4j.websocket.extensions.compress.PerMessageDeflateExtension.NoContext;

public class GpuPerMessageDeflateExtension implements IExtension {

	private static final String CLIENT_NO_CONTEXT = "client_no_context_takeover";
	private static final String SERVER_NO_CONTEXT = "server_no_context_takeover";

	private static final int DEFAULT_LEVEL = 6;

	private final PerMessageDeflateExtension delegate;
	/** null: not negotiated yet; true: the server side (acceptOffer); false: the client side */
	private final Boolean server;
	private final int compressionLevel;

	/** The delegate built with the given compression level. */
	public GpuPerMessageDeflateExtension(PerMessageDeflateExtension delegate, int compressionLevel) {
		this(delegate, null, compressionLevel);
	}

	/** The delegate built with the default compression level (6). */
	public GpuPerMessageDeflateExtension(PerMessageDeflateExtension delegate) {
		this(delegate, null, DEFAULT_LEVEL);
	}

	/** As PerMessageDeflateExtension(compressionLevel, compressNoContext, decompressNoContext). */
	public GpuPerMessageDeflateExtension(int compressionLevel, NoContext compressNoContext,
			NoContext decompressNoContext) {
		this(new PerMessageDeflateExtension(compressionLevel, compressNoContext, decompressNoContext), null,
				compressionLevel);
	}

	public GpuPerMessageDeflateExtension() {
		this(new PerMessageDeflateExtension(), null, DEFAULT_LEVEL);
	}

	private GpuPerMessageDeflateExtension(PerMessageDeflateExtension delegate, Boolean server, int compressionLevel) {
		this.delegate = delegate;
		this.server = server;
		this.compressionLevel = compressionLevel;
	}

	@Override
	public String getName() {
		return delegate.getName();
	}

	@Override
	public Object getGroupId() {
		return delegate.getGroupId();
	}

	@Override
	public IExtension acceptOffer(List<String> offer) throws InvalidExtensionException {
		IExtension e = delegate.acceptOffer(offer);
		return e == null ? null
				: new GpuPerMessageDeflateExtension((PerMessageDeflateExtension) e, Boolean.TRUE, compressionLevel);
	}

	@Override
	public IExtension validateResponse(List<String> response) throws InvalidExtensionException {
		IExtension e = delegate.validateResponse(response);
		return e == null ? null
				: new GpuPerMessageDeflateExtension((PerMessageDeflateExtension) e, Boolean.FALSE, compressionLevel);
	}

	@Override
	public List<String> offer() {
		return delegate.offer();
	}

	@Override
	public List<String> response() {
		return delegate.response();
	}

	@Override
	public void updateEncoders(ICodecPipeline pipeline) {
		delegate.updateEncoders(pipeline);
		ICodec<?, ?> c = pipeline.get(PerMessageDeflateExtension.PERMESSAGE_DEFLATE_ENCODER);
		if (c instanceof PerMessageDeflateEncoder) {
			List<String> r = delegate.response();
			boolean noContext = r.contains(Boolean.TRUE.equals(server) ? SERVER_NO_CONTEXT : CLIENT_NO_CONTEXT);
			GpuPerMessageDeflateEncoder g = new GpuPerMessageDeflateEncoder(compressionLevel, noContext,
					(PerMessageDeflateEncoder) c);
			pipeline.replace(PerMessageDeflateExtension.PERMESSAGE_DEFLATE_ENCODER,
					PerMessageDeflateExtension.PERMESSAGE_DEFLATE_ENCODER, g);
			ICodec<?, ?> w = pipeline.get(IWebSocketSessionConfig.WEBSOCKET_ENCODER);
			if (w instanceof GpuFrameEncoder)
				((GpuFrameEncoder) w).attachDeflate(g);
		}
	}

	@Override
	public void updateDecoders(ICodecPipeline pipeline) {
		delegate.updateDecoders(pipeline);
		ICodec<?, ?> c = pipeline.get(PerMessageDeflateExtension.PERMESSAGE_DEFLATE_DECODER);
		if (c instanceof PerMessageDeflateDecoder) {
			List<String> r = delegate.response();
			boolean noContext = r.contains(Boolean.TRUE.equals(server) ? CLIENT_NO_CONTEXT : SERVER_NO_CONTEXT);
			pipeline.replace(PerMessageDeflateExtension.PERMESSAGE_DEFLATE_DECODER,
					PerMessageDeflateExtension.PERMESSAGE_DEFLATE_DECODER,
					new GpuPerMessageDeflateDecoder(noContext, (PerMessageDeflateDecoder) c));
		}
	}
}

/**
 * The settings of the negotiating handshake natives (wsg_hs_negotiation): the config's
 * supported subprotocols and the two NoContext values of its one
 * PerMessageDeflateExtension.  PerMessageDeflateExtension keeps compressNoContext and
 * decompressNoContext private, so they are given here and not read from a delegate
 * (as the compression level above).  deflate == false: no extension is supported;
 * otherExtensions: the supported list holds anything else, and an extensions field is
 * deferred to the Java Handshaker as before.
 */
final class GpuHandshakeNegotiator {

	private final byte[] image;

	GpuHandshakeNegotiator(String[] subProtocols, boolean deflate, NoContext compressNoContext,
			NoContext decompressNoContext, boolean otherExtensions) {
		image = pack(subProtocols, deflate, compressNoContext, decompressNoContext, otherExtensions);
	}

	/** false: the lists exceed the native caps; the caller sets the config's flags and offers are deferred */
	boolean fits() {
		return image != null;
	}

	/**
	 * The little-endian image of wsg_hs_negotiation: n_protocols, deflate, other_extensions,
	 * compress_no_context, decompress_no_context, 3 reserved bytes; protocol_off[17] (u16) at 8;
	 * protocol_bytes[256] at 48.  null when the subprotocols do not fit (16 entries, 256
	 * bytes, ASCII).
	 */
	static byte[] pack(String[] subProtocols, boolean deflate, NoContext compressNoContext,
			NoContext decompressNoContext, boolean otherExtensions) {
		int n = subProtocols == null ? 0 : subProtocols.length;
		if (n > Wsg.HS_NEG_MAX_PROTOCOLS)
			return null;
		byte[] b = new byte[Wsg.HS_NEGOTIATION_BYTES];
		b[0] = (byte) n;
		b[1] = (byte) (deflate ? 1 : 0);
		b[2] = (byte) (otherExtensions ? 1 : 0);
		b[3] = (byte) (deflate ? compressNoContext.ordinal() : 0); // FORBIDDEN, OPTIONAL, REQUIRED = 0, 1, 2
		b[4] = (byte) (deflate ? decompressNoContext.ordinal() : 0);
		int at = 0;
		for (int k = 0; k < n; ++k) {
			String s = subProtocols[k];
			for (int i = 0; i < s.length(); ++i)
				if (s.charAt(i) > 0x7f)
					return null;
			byte[] p = s.getBytes(StandardCharsets.US_ASCII);
			if (at + p.length > Wsg.HS_NEG_MAX_PROTOCOL_BYTES)
				return null;
			System.arraycopy(p, 0, b, 48 + at, p.length);
			at += p.length;
			b[8 + 2 * (k + 1)] = (byte) at;
			b[9 + 2 * (k + 1)] = (byte) (at >> 8);
		}
		return b;
	}

	/** Handshaker.accept for n requests (Wsg.handshakeAcceptBatchHost's buffers, plus `negotiated`). */
	int accept(long ctx, int[] config, ByteBuffer req, ByteBuffer reqOff, int n, ByteBuffer resp, ByteBuffer result,
			ByteBuffer negotiated) {
		return Wsg.handshakeAcceptNegotiateBatchHost(ctx, config, image, req, reqOff, n, resp, result, negotiated);
	}

	/** Handshaker.validate for n responses (Wsg.handshakeValidateBatchHost's buffers, plus `negotiated`). */
	int validate(long ctx, int[] config, ByteBuffer resp, ByteBuffer respOff, ByteBuffer keys, int n,
			ByteBuffer expected, ByteBuffer result, ByteBuffer negotiated) {
		return Wsg.handshakeValidateNegotiateBatchHost(ctx, config, image, resp, respOff, keys, n, expected, result,
				negotiated);
	}
}
