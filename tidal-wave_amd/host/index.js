// index.js — the JS library API of tidal-wave (reference: /root/reference/index.js:1-72), unchanged in shape:
// create(targetDir, {expectDir | getExpectedPath, ...engine options}) -> EventEmitter with 'data' / 'error' /
// 'finish'.  The reference walks the target directory with `glob-stream`; that module is not installed here,
// so the walk uses fs directly (same '**/*.*' semantics: every file whose name contains a dot).
// Not in the reference: the options `ignore` (an array of {x, y, width, height}, regions of every pair that may differ) or
// `getIgnoreRegions(shortPath)` (a function returning such an array, or nothing, for one pair); a pair with regions goes
// through calcIgnoring, every other pair through calc as before; and `regions` (1 .. 8), which create() hands to the engine with
// the other engine options: every 'data' result then carries `regions` behind `vector`, and every vector its `region`;
// `residual` (1 .. 254) and `residualMin` likewise: every 'data' result then carries `change`, the cells with a pixel that
// differs by more than `residual` gray levels, and a pair with at least `residualMin` unexplained pixels is SUSPICIOUS;
// `shift` (1 .. 1024, the search radius in pixels): every pair's flow starts from its global integer shift, found and checked on the
// device, and every 'data' result carries `shift: {x, y, applied}` behind the other keys; `shiftBands` (32 .. 1024, a multiple of 16, with `shift`): the flow starts
// from one vertical shift per band of that many rows instead, and every 'data' result carries `bands: [{y, rows, dy, applied}, ...]`
// behind `shift`.  `status` is unchanged by it;
// `overlay` (an existing directory) and `overlayTol` (0 .. 255, default 16): every SUSPICIOUS pair's diff image is rendered on the
// device and written there as a PNG, and its 'data' result carries the file's path as `overlay`, the last key.
'use strict';
var EventEmitter = require('events').EventEmitter,
  TidalWave = require('./build/Release/tidalwave').TidalWave,
  Path = require('path'),
  FS = require('fs');
Object.setPrototypeOf(TidalWave.prototype, EventEmitter.prototype);

module.exports.create = create;
module.exports.TidalWave = TidalWave;

function create(targetDir, options) {
  var t = new TidalWave(options);
  options = options || {};

  var getExpectedPath;
  if (typeof options.expectDir === 'string') {
    getExpectedPath = function(shortPath) {
      return Path.resolve(options.expectDir, shortPath);
    };
  } else if (typeof options.getExpectedPath === 'function') {
    getExpectedPath = options.getExpectedPath;
  } else {
    throw new Error('An option must have "expectDir" or "getExpectedPath" property.');
  }

  var getIgnoreRegions = null;
  if (Array.isArray(options.ignore)) {
    getIgnoreRegions = function() { return options.ignore; };
  } else if (typeof options.getIgnoreRegions === 'function') {
    getIgnoreRegions = options.getIgnoreRegions;
  }

  calcAll(t, targetDir, getExpectedPath, getIgnoreRegions);
  return t;
}

function walk(dir, out) {
  var entries;
  try { entries = FS.readdirSync(dir, { withFileTypes: true }); } catch (e) { return out; }
  entries.sort(function(a, b) { return a.name < b.name ? -1 : 1; });
  entries.forEach(function(e) {
    var p = Path.join(dir, e.name);
    if (e.isDirectory()) walk(p, out);
    else if (e.name.indexOf('.') !== -1) out.push(p);
  });
  return out;
}

function calcAll(tidalwave, targetDir, getExpectedPath, getIgnoreRegions) {
  var base = Path.resolve(targetDir);
  var files = walk(base, []);
  var globEnded = false;
  var requested = 0;
  var pending = files.length;

  if (files.length === 0) {
    // index.js:39-44 of the reference: nothing matched -> dispose at once -> 'finish' with zero counts
    setImmediate(function() { tidalwave.dispose(); });
    return;
  }

  files.forEach(function(target) {
    var shortPath = Path.relative(base, target);
    var expectedFile = getExpectedPath.call(this, shortPath);
    if (!expectedFile) { done(); return; }
    if (typeof expectedFile === 'string') calcIfExists(expectedFile);
    else if (typeof expectedFile.then === 'function') expectedFile.then(calcIfExists);
    function calcIfExists(expectedFile) {
      // the reference ignores the result of FS.exists (index.js:57-60): a missing expected file still
      // produces a calc and therefore an ERROR "Can't open ..."
      FS.access(expectedFile, function() {
        var regions = getIgnoreRegions ? getIgnoreRegions.call(this, shortPath) : null;
        if (Array.isArray(regions) && regions.length > 0) tidalwave.calcIgnoring(expectedFile, target, regions);
        else tidalwave.calc(expectedFile, target);
        requested++;
        done();
      });
    }
  });
  var disposed = false;
  function disposeIfIdle() {
    // every requested pair has answered and the walk is over: nothing else will arrive
    if (globEnded && requested <= 0 && !disposed) { disposed = true; tidalwave.dispose(); }
  }
  function done() {
    if (--pending === 0) {
      globEnded = true;
      disposeIfIdle();  // results that came in before the walk ended (or a walk that requested nothing)
    }
  }

  // The reference counts `requested` down only once the walk has ended (`globEnded && --requested <= 0`,
  // index.js:64-68) and, on 'error', never checks for completion (index.js:69-71): an event that arrives before the
  // last FS callback, or a run whose last event is an error, leaves the instance undisposed for ever.  With a
  // millisecond-latency engine both happen, so every event is counted and completion is checked at every step.
  tidalwave.on('data', function() { requested--; disposeIfIdle(); });
  tidalwave.on('error', function() { requested--; disposeIfIdle(); });
}
