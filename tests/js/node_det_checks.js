'use strict';
/* Node-side checks of det, slogdet, det_tri, slogdet_tri, rank, lstsq and norm through the JS host and the N-API addon.
 * Driven by tests/test_node_det.py.
 *   node node_det_checks.js cpu                               (no GPU: argument checks)
 *   node node_det_checks.js install <reference dist/nd.js>    (routing of the seven names, minWork and float32 forwarding)
 *   node node_det_checks.js gpu <golden dir>                  (GPU: results against the reference's goldens; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['det', 'slogdet', 'det_tri', 'slogdet_tri', 'rank', 'lstsq', 'norm'];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: descr === '<f8' ? new Float64Array(ab) : new Int32Array(ab), shape};
}
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

if (mode === 'cpu') {
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  const W = new la.NDArray(Int32Array.of(2, 3), new Float64Array(6));
  assert.throws(() => la.det([1, 2, 3]), /^Error: qr_decomp\(A\): A\.ndim must be at least 2\.$/);
  assert.throws(() => la.det(W), /^Error: det_tri\(a\): a must be square matrices\.$/);
  assert.throws(() => la.slogdet(W), /^Error: det_tri\(A\): A must be square matrices\.$/);
  assert.throws(() => la.det_tri([1, 2]), /^Error: det_tri\(a\): a\.shape=\[2\]; a\.ndim must be at least 2\.$/);
  assert.throws(() => la.slogdet_tri(W), /^Error: det_tri\(A\): A must be square matrices\.$/);
  assert.throws(() => la.norm([1, 2], 'inf'), /^Error: norm\(A,ord,axis\): Unsupported ord: inf\.$/);
  assert.throws(() => la.norm([1, 2], 'fro', 0), /^Error: norm\(A,ord,axis\): axis argument not yet supported\.$/);
  console.log('node det cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {};
  for (const n of NAMES) before[n] = nd.la[n];
  const out = la.install(nd, {minWork: 1e4});
  const L = out.la;
  for (const n of NAMES) { assert.strictEqual(typeof L[n], 'function', n); assert.strictEqual(L.__nd4hip_original__[n], before[n], n); }
  const A3 = nd.array([[2, 1, 0], [1, 3, 1], [0, 1, 4]]);
  assert.strictEqual(L.det(A3).data[0], before.det(A3).data[0]);                 // 3x3: below minWork, forwarded to the host module
  assert.strictEqual(L.norm(A3), before.norm(A3));
  const F = nd.array('float32', [[1, 2], [3, 4]]);
  const full = la.install(require(process.argv[3]), {}).la;                        // no minWork: float32 is still forwarded
  assert.strictEqual(full.det(F).dtype, 'float32');
  assert.strictEqual(full.slogdet_tri(F)[0].dtype, 'float32');
  console.log('node det install checks ok');
} else if (mode === 'gpu') {
  const G = path.join(process.argv[3], 'det');
  const cases = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json'))).cases;
  const arrOf = (meta, key) => { const x = loadNpy(path.join(G, meta.files[key])); return new la.NDArray(Int32Array.from(x.shape), x.data); };
  let n = 0;
  for (const [name, meta] of Object.entries(cases)) {
    if (!meta.stored_input) continue;
    const A = arrOf(meta, 'A');
    for (const op of ['det_tri', 'det']) {
      if (!meta.ops[op] || meta.ops[op].error) continue;
      if (op === 'det' && !(A.shape[A.ndim - 1] === A.shape[A.ndim - 2] && A.shape[A.ndim - 1] <= 64)) continue;
      const d = la[op](A), ref = arrOf(meta, op);
      assert.deepStrictEqual(Array.from(d.shape), Array.from(ref.shape), name);
      assert(sameBits(d.data, ref.data), `${name} ${op}`);                          // bit-identical tiers
      const dd = la[op](la.to_device(A));
      assert(dd instanceof la.DeviceNDArray && sameBits(dd.data, ref.data), `${name} ${op} device`);
      n++;
    }
    for (const op of ['det', 'slogdet']) if (meta.ops[op] && meta.ops[op].error) assert.throws(() => la[op](A), e => e.message.endsWith(meta.ops[op].error), name);
    if (meta.ops.norm) {
      const v = la.norm(A), ref = arrOf(meta, 'norm').data[0];
      assert(Number.isFinite(ref) ? Math.abs(v - ref) <= 1e-13 * ref : Object.is(v, ref), name);
      assert(Object.is(la.norm(la.to_device(A)), v), name + ' device');
      n++;
    }
    if (meta.ops.rank) {
      assert.deepStrictEqual(Array.from(la.rank(A).data), Array.from(arrOf(meta, 'rank').data), name);
      const x = la.lstsq(A, arrOf(meta, 'y')), ref = arrOf(meta, 'lstsq');
      let dn = 0, rn = 0; for (let i = 0; i < ref.data.length; i++) { dn += (x.data[i] - ref.data[i]) ** 2; rn += ref.data[i] ** 2; }
      assert(Math.sqrt(dn) <= 1e-10 * Math.max(Math.sqrt(rn), 1), name);
      n++;
    }
  }
  assert(n > 40, n);
  console.log('node det gpu checks ok', n);
} else throw new Error('mode');
