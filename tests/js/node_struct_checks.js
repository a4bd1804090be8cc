'use strict';
/* Node-side checks of the structure functions (tril, triu, diag, diag_mat, permute_rows, permute_cols, unpermute_rows,
 * unpermute_cols) and of DeviceNDArray.T through the JS host and the N-API addon. Driven by tests/test_node_struct.py.
 *   node node_struct_checks.js cpu <golden dir>                  (no GPU: every refused call of the manifest with its recorded text)
 *   node node_struct_checks.js install <reference dist/nd.js>    (routing of the eight names: host arguments of any dtype get the host
 *                                                                 module's own function and result)
 *   node node_struct_checks.js gpu <golden dir>                  (GPU: the fixtures bit for bit on host and on device arrays, .T,
 *                                                                 nothing downloaded by a device call; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['tril', 'triu', 'diag', 'diag_mat', 'permute_rows', 'permute_cols', 'unpermute_rows', 'unpermute_cols'];
const PERM = NAMES.slice(4);

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: descr === '<i4' ? new Int32Array(ab) : new Float64Array(ab), shape};
}
// equal in every bit, where NaN equals any NaN
function sameBits(a, b, what) {
  assert.strictEqual(a.length, b.length, what);
  for (let i = 0; i < a.length; i++) assert(Object.is(a[i], b[i]), `${what}: entry ${i} is ${a[i]}, the reference has ${b[i]}`);
}
const prod = s => s.reduce((x, y) => x * y, 1);
function fixtures(dir) {
  const G = path.join(dir, 'struct'), m = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json')));
  return {m, load: entry => loadNpy(path.join(G, entry.file))};
}
// the arguments of a refused call, built by `make(shape, typed)`
function refusedArgs(e, make) {
  const A = make(e.a_shape, new Float64Array(prod(e.a_shape)));
  if (!PERM.includes(e.fn)) return e.fn === 'diag' ? [A, e.offset] : [A];
  const n = prod(e.p_shape), L = e.p_shape.length ? e.p_shape[e.p_shape.length - 1] : 1;
  const P = e.p_dtype === 'int32' ? make(e.p_shape, e.p_values ? Int32Array.from(e.p_values) : Int32Array.from({length: n}, (_, i) => i % L))
                                  : make(e.p_shape, new Float64Array(n));
  return [A, P];
}

if (mode === 'cpu') {
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  const {m} = fixtures(process.argv[3]);
  const make = (shape, data) => new la.NDArray(Int32Array.from(shape), data);
  let n = 0;
  for (const e of m.errors) {
    if (e.on_device) continue;
    // a P that is not int32 has no accelerated form: standalone there is no host module to hand it to
    const want = e.p_dtype === 'float64' ? `nd4hip.${e.fn}: dtype is not accelerated.` : e.message;
    assert.throws(() => la[e.fn](...refusedArgs(e, make)), err => err.message === want, `${e.fn} ${JSON.stringify(e.a_shape)}: expected "${want}"`);
    n++;
  }
  assert(n >= 30);
  for (const fn of ['tril', 'triu', 'diag', 'diag_mat'])
    assert.throws(() => la[fn](make([2, 2], new Float32Array(4))), new RegExp(`^Error: nd4hip\\.${fn}: dtype is not accelerated\\.$`));
  for (const fn of PERM)
    assert.throws(() => la[fn](make([2, 2], new Int32Array(4)), make([2], Int32Array.of(0, 1))), new RegExp(`^Error: nd4hip\\.${fn}: dtype is not accelerated\\.$`));
  // the shape rules of .T (building a DeviceNDArray needs a device, so they are a static function that .T goes through)
  assert('T' in la.DeviceNDArray.prototype);
  const tShape = la.DeviceNDArray.transposedShape;
  assert.strictEqual(tShape(Int32Array.of(), 'float64'), null);                  // fewer than two axes: the array itself, any dtype
  assert.strictEqual(tShape(Int32Array.of(7), 'int32'), null);
  assert.deepStrictEqual(Array.from(tShape(Int32Array.of(5, 8), 'float64')), [8, 5]);
  assert.deepStrictEqual(Array.from(tShape(Int32Array.of(2, 3, 1, 9), 'float64')), [2, 3, 9, 1]);
  for (const dtype of ['int32', 'complex128'])
    assert.throws(() => tShape(Int32Array.of(2, 2), dtype), new RegExp(`^Error: nd4hip\\.T: ${dtype} device arrays are not accelerated\\.$`));
  console.log('node struct cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {};
  for (const n of NAMES) before[n] = nd.la[n];
  const L = la.install(nd, {minWork: 1e12}).la;                       // minWork plays no part for these names
  for (const n of NAMES) { assert.strictEqual(typeof L[n], 'function', n); assert.strictEqual(L.__nd4hip_original__[n], before[n], n); assert.notStrictEqual(L[n], before[n], n); assert.strictEqual(L[n].name, n); }
  // host arguments of any dtype: the host module's own result, dtype included
  const vals = [[1, -0, NaN, 4], [5, 6, -Infinity, 8], [9, 10, 11, 12]];
  const P3 = nd.array('int32', [2, 0, 2]), P4 = nd.array('int32', [3, 3, 0, 1]);
  for (const dtype of ['float64', 'float32', 'int32']) {
    const A = nd.array(dtype, dtype === 'int32' ? [[1, 0, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]] : vals), d = nd.array(dtype, [1, 2, 3]);
    const calls = {tril: [A, -1], triu: [A, 1], diag: [A, 1], diag_mat: [d], permute_rows: [A, P3], unpermute_rows: [A, P3], permute_cols: [A, P4], unpermute_cols: [A, P4]};
    for (const n of NAMES) {
      const got = L[n](...calls[n]), want = before[n](...calls[n]);
      assert.strictEqual(got.dtype, dtype, `${n} ${dtype}`);
      assert.strictEqual(got.dtype, want.dtype);
      assert.deepStrictEqual(Array.from(got.shape), Array.from(want.shape), n);
      sameBits(got.data, want.data, `${n} ${dtype}`);
    }
  }
  // the host module's own refusals come through untouched
  const {m} = fixtures(process.argv[4]);
  for (const e of m.errors) {
    const make = (shape, data) => new nd.NDArray(Int32Array.from(shape), data);
    assert.throws(() => L[e.fn](...refusedArgs(e, make)), err => err.message === e.message, `${e.fn}: expected "${e.message}"`);
  }
  console.log('node struct install checks ok');
} else if (mode === 'gpu') {
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof Float64Array ? 'float64' : this.data instanceof Int32Array ? 'int32' : this.data instanceof Float32Array ? 'float32' : 'object'; }
  }
  const L = la.install({NDArray: HostNDArray, la: {matmul2: () => 'host'}}).la;
  const {m, load} = fixtures(process.argv[3]);
  const host = x => new HostNDArray(Int32Array.from(x.shape), x.data);
  let n = 0;
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name], want = load(c.out);
    const A = load(m.inputs[c.args.A]), P = c.args.P ? load(m.inputs[c.args.P]) : null;
    const rest = P ? [] : ['k', 'offset'].filter(k => k in c.args).map(k => c.args[k]);
    if (c.fn === 'transpose') {
      const dA = L.to_device(host(A)), T = dA.T;
      assert(T instanceof L.DeviceNDArray && dA._host === null, name);
      assert.deepStrictEqual(Array.from(T.shape), want.shape, name);
      sameBits(T.data, want.data, name);
      sameBits(T.T.data, A.data, name + ' .T.T');
      n++;
      continue;
    }
    // host arrays: the standalone path (upload, run, download)
    const h = L[c.fn](host(A), ...(P ? [host(P)] : rest));
    assert(h instanceof HostNDArray, name);
    assert.deepStrictEqual(Array.from(h.shape), want.shape, name);
    sameBits(h.data, want.data, name + ' (host arrays)');
    // device arrays: device arrays out, nothing downloaded
    const dA = L.to_device(host(A)), dP = P ? L.to_device(host(P)) : null;
    const d = L[c.fn](dA, ...(P ? [dP] : rest));
    assert(d instanceof L.DeviceNDArray && dA._host === null && (!dP || dP._host === null) && d._host === null, name + ': a device call downloaded');
    assert.deepStrictEqual(Array.from(d.shape), want.shape, name);
    sameBits(d.data, want.data, name + ' (device arrays)');
    if (P && n % 3 === 0) {           // a host operand next to a device one is uploaded on the way in
      sameBits(L[c.fn](dA, host(P)).data, want.data, name + ' (host P)');
      sameBits(L[c.fn](host(A), dP).data, want.data, name + ' (host A)');
    }
    n++;
  }
  assert(n >= 100);
  // fewer than two axes: the array itself; complex and int32 device arrays are refused
  const v = L.to_device(host({shape: [3], data: Float64Array.of(1, 2, 3)}));
  assert.strictEqual(v.T, v);
  assert.throws(() => L.to_device(host({shape: [1, 3], data: Int32Array.of(1, 2, 3)})).T, /not accelerated/);
  // a device argument of a dtype that has no device form is refused, never handed to a host function (that would download it)
  { const hostCalls = [];
    const L2 = la.install({NDArray: HostNDArray, la: {matmul2: () => 'host', tril: (...a) => { hostCalls.push(a); return 'host'; },
                                                        permute_rows: (...a) => { hostCalls.push(a); return 'host'; }}}).la;
    const dI = L2.to_device(host({shape: [2, 2], data: Int32Array.of(1, 2, 3, 4)})), dF = L2.to_device(host({shape: [2], data: Float64Array.of(0, 1)}));
    const dA = L2.to_device(host({shape: [2, 2], data: Float64Array.of(1, 2, 3, 4)}));
    assert.throws(() => L2.tril(dI), /^Error: nd4hip\.tril: dtype is not accelerated\.$/);
    assert.throws(() => L2.permute_rows(dA, dF), /^Error: nd4hip\.permute_rows: dtype is not accelerated\.$/);
    assert(hostCalls.length === 0 && dI._host === null && dF._host === null && dA._host === null);
    assert.strictEqual(L2.tril(host({shape: [2, 2], data: Int32Array.of(1, 2, 3, 4)})), 'host'); }
  // an index out of range on device arrays: the recorded text, and the handle stays usable
  for (const e of m.errors) {
    if (!e.on_device) continue;
    const make = (shape, data) => L.to_device(new HostNDArray(Int32Array.from(shape), data));
    assert.throws(() => L[e.fn](...refusedArgs(e, make)), err => err.message === e.message, `${e.fn}: expected "${e.message}"`);
  }
  sameBits(L.to_device(host(load(m.inputs.A_5x8))).T.T.data, load(m.inputs.A_5x8).data, 'after the refused calls');
  console.log('node struct gpu checks ok');
} else throw new Error('mode');
